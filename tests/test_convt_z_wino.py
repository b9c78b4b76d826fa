"""The Winograd-domain Z form of the last up-sampling layer (tg_convt3x3s2_z_wino_fwd, tg_convt3x3s2_wino.hip):
F(2,2) along x and y over 2x2 input tiles, 25 products per tile instead of 36, with conv_out's channel contraction in the
epilogue.  Checked against the fp64 composition (ConvTranspose2d + ReLU, then the tap planes of the output conv), against
the direct Z form's own error, for grid independence (split / unsplit launch, n = 2 against two n = 1 calls), and through
the default frame plan, whose HR frame must be this op's composition bit for bit."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

T = torch.from_numpy


def dev(x):
    return x.cuda().contiguous()


def rs(seed, shape, lo=0.0, hi=1.0):
    return T(np.random.RandomState(seed).uniform(lo, hi, shape).astype(np.float32))


@pytest.fixture(scope='module')
def ops():
    import tecogan_pytorch_amd.ops as ops_
    return ops_


def _case(ops, n, cin, cout, cz, h, w, scale=1.0, seed=1):
    import torch.nn.functional as F
    x = rs(seed, (n, cin, h, w), -1, 1) * scale
    wt = rs(seed + 1, (cin, cout, 3, 3), -1, 1) / (1.5 * cin ** 0.5)
    b = rs(seed + 2, (cout,), -0.5, 0.5) * scale
    wo = rs(seed + 3, (cz, cout, 3, 3), -1, 1) / (3.0 * cout ** 0.5)
    up = torch.relu(F.conv_transpose2d(x.double(), wt.double(), b.double(), stride=2, padding=1, output_padding=1))
    ref = torch.einsum('octk,nchw->ntkohw', wo.double().reshape(cz, cout, 3, 3), up).reshape(n, 9 * cz, 2 * h, 2 * w)
    pk, _, _, _ = ops.pack_conv3x3(dev(wt), transposed=True)
    wa = ops.convt_pack_wino(pk, cin, cout)
    wz = ops.convt_pack_wz(dev(wo))
    return dev(x), pk, wa, dev(b), wz, ref


def _errs(out, ref):
    d = (out.detach().cpu().double() - ref).abs()
    return d.max().item(), d.mean().item()


@pytest.mark.parametrize('n,cz,h,w', [(1, 3, 12, 20), (2, 3, 7, 35), (1, 3, 33, 64), (2, 1, 21, 70), (1, 2, 9, 33),
                                      (1, 3, 70, 130), (1, 3, 268, 640)])
def test_wino_z_matches_the_composition(ops, n, cz, h, w):
    """Ragged shapes (w not a multiple of 32, odd h and w, n = 2, cz = 1..3) and the 268x640 frame: within 1e-5 of the
    fp64 composition, planes past 9 cz untouched."""
    x, pk, wa, b, wz, ref = _case(ops, n, 64, 64, cz, h, w)
    out = torch.full((n, 32, 2 * h, 2 * w), 7.0, device='cuda')
    ops.convt3x3s2_z_wino(x, wa, b, wz, cz, 64, act=1, out=out)
    e, _ = _errs(out[:, :9 * cz], ref)
    assert e <= 1e-5, e
    assert bool((out[:, 9 * cz:] == 7.0).all()), 'the Winograd form wrote outside its planes'


@pytest.mark.parametrize('scale', [1.0, 1e2, 1e3])
def test_wino_z_error_is_at_most_twice_the_direct_forms(ops, scale):
    """Maximum and mean error against fp64 at most 2x the direct Z form's, including at trained-activation magnitudes
    (inputs and bias scaled to 1e2..1e3)."""
    n, cz, h, w = 1, 3, 70, 130
    x, pk, wa, b, wz, ref = _case(ops, n, 64, 64, cz, h, w, scale=scale, seed=11)
    wino = ops.convt3x3s2_z_wino(x, wa, b, wz, cz, 64, act=1)[:, :9 * cz]
    direct = ops.convt3x3s2_z(x, pk, b, wz, cz, 64, act=1, form=0)[:, :9 * cz]
    ew, mw = _errs(wino, ref)
    ed, md = _errs(direct, ref)
    assert ew <= 2 * ed and mw <= 2 * md, (scale, ew, ed, mw, md)


def test_wino_z_split_and_batch_are_bit_identical(ops):
    """The two-launch split (whole rounds of workgroups + a remainder) equals one launch bit for bit at the 268x640 frame;
    n = 2 equals two n = 1 calls bit for bit."""
    n, cz, h, w = 1, 3, 268, 640
    x, pk, wa, b, wz, _ = _case(ops, n, 64, 64, cz, h, w, seed=21)
    one = ops.convt3x3s2_z_wino(x, wa, b, wz, cz, 64, act=1, split=0)
    for split in (1, -1):
        out = torch.full((n, 32, 2 * h, 2 * w), 7.0, device='cuda')
        ops.convt3x3s2_z_wino(x, wa, b, wz, cz, 64, act=1, split=split, out=out)
        assert torch.equal(out[:, :27], one[:, :27]), (split, (out[:, :27] - one[:, :27]).abs().max().item())
        assert bool((out[:, 27:] == 7.0).all()), split
    x2, _, wa2, b2, wz2, _ = _case(ops, 2, 64, 64, cz, 37, 70, seed=31)
    both = ops.convt3x3s2_z_wino(x2, wa2, b2, wz2, cz, 64, act=1)
    for i in range(2):
        single = ops.convt3x3s2_z_wino(x2[i:i + 1].contiguous(), wa2, b2, wz2, cz, 64, act=1)
        assert torch.equal(both[i:i + 1, :27], single[:, :27]), i


def test_default_plan_runs_the_wino_z_form():
    """The default 134x320 4x plan: its Z-stage input (the first up-sampling layer's output, left in the workspace)
    through ops.convt3x3s2_z_wino + ops.convout_tail reproduces the plan's tap planes and HR frame bit for bit, and the
    direct Z form does not."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, 'tests', 'golden'))
    from procedural_weights import generator_state_dict, smooth_clip
    from tecogan_pytorch_amd import ops
    from tecogan_pytorch_amd import _lib as L
    from tecogan_pytorch_amd.models.networks import FRNet
    deg, s, h, w = 'BD', 4, 134, 320
    net = FRNet(3, 3, 64, 10, deg, s)
    net.load_state_dict(generator_state_dict(scale=s, degradation=deg), strict=True)
    net = net.cuda().eval()
    clip = smooth_clip(2, 3, h, w, seed=57, shift=1.1)
    lr_curr, lr_prev = clip[1:2].cuda().contiguous(), clip[0:1].cuda().contiguous()
    hr_prev = torch.rand(1, 3, s * h, s * w, generator=torch.Generator().manual_seed(3)).cuda()
    with torch.no_grad():
        out = net.step(lr_curr, lr_prev, hr_prev)
    torch.cuda.synchronize()
    net.check_faults()
    plan = net._get_plan(1, h, w, torch.device('cuda', 0))
    lib = L.lib()
    names = {}
    for k in range(lib.tg_frnet_plan_kinds()):
        nl = ctypes.c_int()
        L.check(lib.tg_frnet_plan_kind_stats(plan.handle, k, ctypes.byref(nl), None, None), 'kind_stats')
        names[lib.tg_frnet_kind_name(k).decode()] = nl.value
    assert names['convt3x3s2_mfma_kernel<Z>'] == 2, names
    # workspace regions of tg_api.hip's carve(): A, B, FLOW, S2D, U1 (the Z input), U2 (the planes), 64-float aligned
    hw = h * w

    def a64(v):
        return (v + 63) // 64 * 64
    off_u1 = 2 * a64(64 * hw) + a64(2 * hw) + a64(s * s * 3 * hw)
    off_u2 = off_u1 + a64(64 * 4 * hw)
    ws = plan.workspace
    zin = ws[off_u1:off_u1 + 64 * 4 * hw].view(1, 64, 2 * h, 2 * w)
    planes = ws[off_u2:off_u2 + 32 * s * s * hw].view(1, 32, s * h, s * w)
    up1, up2, conv_out = net.srnet.layers()[-3:]
    pk = up2.packed()[0]
    wa = ops.convt_pack_wino(pk, 64, 64)
    wz = ops.convt_pack_wz(conv_out.weight.detach().contiguous())
    b2 = up2.bias.detach().contiguous()
    z = ops.convt3x3s2_z_wino(zin.contiguous(), wa, b2, wz, 3, 64, act=ops.ACT_RELU)
    assert torch.equal(z[:, :27], planes[:, :27]), (z[:, :27] - planes[:, :27]).abs().max().item()
    hr = ops.convout_tail(z, 3, conv_out.bias.detach().contiguous(), up_src=lr_curr, up_mode=ops.UP_BICUBIC, up_scale=s)
    assert torch.equal(hr, out), (hr - out).abs().max().item()
    direct = ops.convt3x3s2_z(zin.contiguous(), pk, b2, wz, 3, 64, act=ops.ACT_RELU)
    assert not torch.equal(direct[:, :27], planes[:, :27])
    assert (direct[:, :27] - planes[:, :27]).abs().max().item() <= 1e-4
