"""One process, two devices: what the launch layer (csrc/tg_launch.h) remembers -- a kernel's dynamic-LDS opt-in, the CU
count, how many persistent workgroups fit at once -- belongs to a device.  Each case runs on cuda:1 FIRST and on cuda:0
second, so that whatever the first device left behind is there when the second one asks; both must compute the same
bits.  Skipped on a machine with one GPU: a guard, the proof is the CPU test of the table (tests/test_launch_table_cpu.py)."""
import numpy as np
import pytest
import torch

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(torch.cuda.device_count() < 2, reason='needs two GPUs in one process')]

from procedural_weights import generator_state_dict, smooth_clip

ORDER = ('cuda:1', 'cuda:0')


def rs(seed, shape, lo=0.0, hi=1.0):
    return torch.from_numpy(np.random.RandomState(seed).uniform(lo, hi, shape).astype(np.float32))


def test_conv3x3_with_more_than_64_kb_of_lds_on_both_devices():
    """n=1, cin=128, cout=64, 16x32 takes the in-workgroup K-split kernel (16 chunks: not the one-shot form), whose dynamic
    LDS is 2 * 2 * (3 * 2 * 34 * 4 + 9 * 8 * 64) * 4 = 86,784 bytes: above the 64 KB a kernel gets without the opt-in.
    ksplit=1 is tg_conv3x3_fwd itself (left to the library's heuristic this shape goes to the split-K pair of launches).
    Tolerance against fp64 F.conv2d: that of test_hip_parity.test_conv3x3_mfma."""
    import torch.nn.functional as F
    import tecogan_pytorch_amd.ops as ops
    n, cin, cout, h, w = 1, 128, 64, 16, 32
    x = rs(1, (n, cin, h, w), -1, 1)
    wt = rs(2, (cout, cin, 3, 3), -1, 1) / (3.0 * cin ** 0.5)
    b = rs(3, (cout,), -0.5, 0.5)
    ref = torch.relu(F.conv2d(x.double(), wt.double(), b.double(), padding=1))
    outs = []
    for d in ORDER:
        with torch.cuda.device(d):
            pk, _, _, ocb = ops.pack_conv3x3(wt.to(d))
            out = ops.conv3x3(x.to(d), pk, b.to(d), cin, cout, ocb, 1, ksplit=1)
            torch.cuda.synchronize()
        e = (out.cpu().double() - ref).abs().max().item()
        print(f'{d}: max abs err vs fp64 conv2d {e:.2e}')
        assert e <= 1e-5, (d, e)
        outs.append(out.cpu())
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))


def test_resident_body_frame_on_both_devices():
    """One FRNet.step at the smallest resident-body shape of tests/plan_matrix.py (ct0_res_64x160: nf 64, nb 2, 4x BD, one
    64x160 frame): the grid of the resident launch is sized from the device's capacity."""
    from tecogan_pytorch_amd.models.networks import FRNet
    nf, nb, s, deg, h, w = 64, 2, 4, 'BD', 64, 160
    sd = generator_state_dict(nf=nf, nb=nb, scale=s, degradation=deg)
    clip = smooth_clip(2, 3, h, w, seed=11)
    hp = smooth_clip(1, 3, s * h, s * w, seed=31, shift=0.0)
    outs = []
    for d in ORDER:
        with torch.cuda.device(d), torch.no_grad():
            net = FRNet(3, 3, nf, nb, deg, s)
            net.load_state_dict(sd, strict=True)
            net = net.to(d).eval()
            out = net.step(clip[1:2].to(d), clip[0:1].to(d), hp.to(d))
            torch.cuda.synchronize()
            plan = net._get_plan(1, h, w, torch.device(d))
            plan.check_chain()
            state = plan.chain_state()
        print(f'{d}: chain_state {state}')
        assert state[0] == 0, (d, state)
        assert torch.isfinite(out).all().item()
        outs.append(out.cpu())
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
