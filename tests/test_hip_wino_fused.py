"""The memory-bound neighbours of a Winograd conv folded into its kernel (tg_conv3x3_wino_fused_fwd, tg_conv3x3_wino.hip):
MaxPool2d(2, 2) as the epilogue (POOL) and the bilinear x2 up-sampling as the input staging (UP2).  Both are checked bit
for bit against the two separate launches they replace, at the smallest maps that reach every tile arrangement of the
kernel (TR = 1 / 2 / 4), a ragged last tile column, two output-channel groups, a padded K stage and a padded
output-channel block (cout = 32); the up-sampling kernels themselves against their results from before they shared
their blend expression with the conv (tests/golden/upsample_bilinear_unshared.npz); and through an FNet-only frame plan
whose flow must equal the composition of the separate ops, with no pool / up-sampling launch left beside a Winograd
neighbour."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_DIR = os.path.join(ROOT_DIR, 'tests', 'golden')

T = torch.from_numpy
LRELU = 2

# conv maps (h, w) and the tile arrangement the launcher picks for them (fewest workgroups, ties to the widest):
# 4x6 -> TR 2, 6x34 -> TR 4 (ragged last column), 10x8 -> TR 4, 12x16 -> TR 2, 2x34 and 4x64 -> TR 1 (one / two tile rows)
MAPS = [(4, 6), (6, 34), (10, 8), (12, 16), (2, 34), (4, 64)]
# (cin, cout): one K stage; K padded 20 -> 32 and two output-channel groups; a zero-padded output-channel block
CHANNELS = [(16, 64), (20, 128), (32, 32), (64, 32)]


def dev(x):
    return x.cuda().contiguous()


def rs(seed, shape, lo=0.0, hi=1.0):
    return T(np.random.RandomState(seed).uniform(lo, hi, shape).astype(np.float32))


@pytest.fixture(scope='module')
def ops():
    import tecogan_pytorch_amd.ops as ops_
    from tecogan_pytorch_amd import _lib
    _lib.lib()
    return ops_


_layers = {}


def layer(ops, cin, cout):
    """(weights, bias, packed U) of a layer, made once per channel pair."""
    if (cin, cout) not in _layers:
        wt = rs(2, (cout, cin, 3, 3), -1, 1) / (3.0 * cin ** 0.5)
        b = rs(3, (cout,), -0.5, 0.5)
        _layers[(cin, cout)] = (wt, b, ops.pack_conv3x3_wino(dev(wt)), dev(b))
    return _layers[(cin, cout)]


def ref64(x, wt, b, act):
    import torch.nn.functional as F
    r = F.conv2d(x.double(), wt.double(), b.double(), padding=1)
    return torch.where(r >= 0, r, r * 0.2) if act == LRELU else r


@pytest.mark.parametrize('h,w', MAPS)
@pytest.mark.parametrize('cin,cout', CHANNELS)
def test_pool_epilogue_equals_conv_then_maxpool(ops, cin, cout, h, w):
    wt, b, u, bd = layer(ops, cin, cout)
    x = dev(rs(1, (2, cin, h, w), -1, 1))
    for act in (LRELU, 0):
        want = ops.maxpool2(ops.conv3x3_wino(x, u, bd, cin, cout, act))
        got = ops.conv3x3_wino(x, u, bd, cin, cout, act, pool=True)
        assert got.shape == (2, cout, h // 2, w // 2) and torch.equal(got, want), (act, (got - want).abs().max().item())
    # a strided destination (a slice of a larger batch buffer): y_nstride is the pooled tensor's
    big = torch.full((2, cout + 3, h // 2, w // 2), 7.0, device='cuda')
    ops.conv3x3_wino(x, u, bd, cin, cout, 0, pool=True, out=big[:, :cout])
    assert torch.equal(big[:, :cout], want) and bool((big[:, cout:] == 7.0).all())
    if cout == 32:      # the zero-padded block against fp64, the tolerance of the 64-channel layer test
        import torch.nn.functional as F
        r = F.max_pool2d(ref64(x.cpu(), wt, b, 0), 2)
        assert (got.cpu().double() - r).abs().max().item() <= 1e-5


@pytest.mark.parametrize('h,w', MAPS)
@pytest.mark.parametrize('cin,cout', CHANNELS)
def test_up2_staging_equals_upsample_then_conv(ops, cin, cout, h, w):
    wt, b, u, bd = layer(ops, cin, cout)
    src = dev(rs(5, (2, cin, h // 2, w // 2), -1, 1))
    up = ops.upsample(src, 2, ops.UP_BILINEAR)
    want = ops.conv3x3_wino(up, u, bd, cin, cout, LRELU)
    got = ops.conv3x3_wino(src, u, bd, cin, cout, LRELU, up2=True)
    assert got.shape == (2, cout, h, w) and torch.equal(got, want), (got - want).abs().max().item()
    if cout == 32:
        assert (got.cpu().double() - ref64(up.cpu(), wt, b, LRELU)).abs().max().item() <= 1e-5


@pytest.mark.parametrize('h,w', MAPS + [(5, 9)])
@pytest.mark.parametrize('cin,cout', [(32, 32), (64, 32), (20, 20)])
def test_32_channel_workgroup_equals_the_64_channel_one_on_the_padded_pack(ops, cin, cout, h, w):
    """cout <= 32 runs the workgroup of 2 output-channel waves x 2 tile groups; the 64-channel workgroup called with
    cout = 64 on the same zero-padded pack (and a zero-padded bias) is the kernel as it was: bit-identical, plain, with
    POOL, with UP2, and with two sources + residual; against fp64 within the tolerance of the 64-channel layer test."""
    wt, b, u, bd = layer(ops, cin, cout)
    b64 = torch.zeros(64, device='cuda')
    b64[:cout] = bd
    x = dev(rs(1, (2, cin, h, w), -1, 1))
    got = ops.conv3x3_wino(x, u, bd, cin, cout, LRELU)
    assert torch.equal(got, ops.conv3x3_wino(x, u, b64, cin, 64, LRELU)[:, :cout])
    assert (got.cpu().double() - ref64(x.cpu(), wt, b, LRELU)).abs().max().item() <= 1e-5
    res = dev(rs(4, (2, cout, h, w), -1, 1))
    res64 = torch.zeros(2, 64, h, w, device='cuda')
    res64[:, :cout] = res
    c1 = cin // 2 + 3
    xa, xb = x[:, :c1].contiguous(), x[:, c1:].contiguous()
    assert torch.equal(ops.conv3x3_wino(xa, u, bd, cin, cout, 1, x2=xb, res=res),
                       ops.conv3x3_wino(xa, u, b64, cin, 64, 1, x2=xb, res=res64)[:, :cout])
    if h % 2 == 0 and w % 2 == 0:
        assert torch.equal(ops.conv3x3_wino(x, u, bd, cin, cout, LRELU, pool=True),
                           ops.conv3x3_wino(x, u, b64, cin, 64, LRELU, pool=True)[:, :cout])
        src = dev(rs(5, (2, cin, h // 2, w // 2), -1, 1))
        assert torch.equal(ops.conv3x3_wino(src, u, bd, cin, cout, LRELU, up2=True),
                           ops.conv3x3_wino(src, u, b64, cin, 64, LRELU, up2=True)[:, :cout])


def test_fused_forms_refuse_what_they_do_not_cover(ops):
    from tecogan_pytorch_amd import _lib as L
    wt, b, u, bd = layer(ops, 16, 64)
    for h, w in ((5, 6), (6, 5), (1, 2)):          # odd (or no whole tile): the plan keeps the separate pool launch
        with pytest.raises(L.TecoganHipError):
            ops.conv3x3_wino(dev(rs(1, (1, 16, h, w))), u, bd, 16, 64, 0, pool=True)
    x = dev(rs(1, (1, 16, 4, 6)))
    with pytest.raises(L.TecoganHipError):          # the two flags together
        ops.conv3x3_wino(x, u, bd, 16, 64, 0, pool=True, up2=True)
    for kw in (dict(res=dev(rs(2, (1, 64, 4, 6)))), dict(mask=dev(rs(2, (1, 64, 4, 6)))), dict(x2=x)):
        for fuse in (dict(pool=True), dict(up2=True)):
            with pytest.raises(L.TecoganHipError):
                ops.conv3x3_wino(x, u, bd, 16 if 'x2' not in kw else 32, 64, 0, **kw, **fuse)
    lib = L.lib()
    y = torch.empty(1, 64, 4, 6, device='cuda')
    args = (x.data_ptr(), 16 * 24, u.data_ptr(), bd.data_ptr(), y.data_ptr(), 64 * 24, 1, 16, 64, 4, 6, 0)
    assert lib.tg_conv3x3_wino_fused_fwd(*args, 4, None) != 0           # an unknown flag
    assert lib.tg_conv3x3_wino_fused_fwd(*args, 0, None) == 0           # no flag: the plain kernel
    torch.cuda.synchronize()
    assert torch.equal(y, ops.conv3x3_wino(x, u, bd, 16, 64, 0))


def test_upsampling_kernels_kept_their_bits(ops):
    """ops.upsample against its own results recorded before bilinear_blend was shared with the conv's staging: the x2
    kernel (even width), the general kernel (odd width, x4) and the output multiplier."""
    g = np.load(os.path.join(GOLDEN_DIR, 'upsample_bilinear_unshared.npz'))
    names = sorted(k[2:] for k in g.files if k.startswith('x_'))
    assert len(names) >= 6
    for k in names:
        scale, mul = int(g['scale_' + k]), float(g['mul_' + k])
        got = ops.upsample(dev(T(g['x_' + k])), scale, ops.UP_BILINEAR, mul)
        assert np.array_equal(got.cpu().numpy().view(np.uint32), g['y_' + k].view(np.uint32)), k


_PLAN_CHILD = r"""
import ctypes, sys, torch
sys.path.insert(0, %r); sys.path.insert(0, %r)
from tests.test_hip_parity import make_net, smooth_clip
from tecogan_pytorch_amd import _lib as L, ops
lib = L.lib()
net, _ = make_net('BD', 4)
names = [lib.tg_frnet_kind_name(k).decode() for k in range(lib.tg_frnet_plan_kinds())]
A = ops.ACT_LRELU02
f = net.fnet

def run(n, h, w):
    lr = smooth_clip(n + 1, 3, h, w, seed=11).cuda().contiguous()
    cur, prev = lr[1:].contiguous(), lr[:-1].contiguous()
    plan = net._get_plan(n, h, w, torch.device('cuda'), fnet_only=True)
    st = torch.cuda.current_stream().cuda_stream
    L.check(lib.tg_frnet_step_phase(plan.handle, 1, 0, cur.data_ptr(), prev.data_ptr(), None, None, None, st), 'phase1')
    torch.cuda.synchronize()
    fh, fw = h // 8 * 8, w // 8 * 8
    off = (lib.tg_frnet_plan_flow(plan.handle, 0) - plan.workspace.data_ptr()) // 4      # the flow slot lies in the workspace
    flow = plan.workspace[off:off + n * 2 * fh * fw].view(n, 2, fh, fw).clone()
    def launches(kind):
        v = ctypes.c_int()
        L.check(lib.tg_frnet_plan_kind_stats(plan.handle, names.index(kind), ctypes.byref(v), None, None), 'kind_stats')
        return v.value
    # the same layers from separate ops: conv (the form the plan's rule picks), then the pool / up-sampling launch
    def wino(m, hh, ww):
        return m.packed_wino() is not None and bool(lib.tg_conv3x3_prefers_wino(n, m.cin, m.cout, hh, ww))
    def conv(m, x, x2=None):
        if wino(m, x.shape[2], x.shape[3]):
            return ops.conv3x3_wino(x, m.packed_wino(), m.bias.detach(), m.cin, m.cout, A, x2=x2)
        pk, ocb = m.packed()
        return ops.conv3x3(x, pk, m.bias.detach(), m.cin, m.cout, ocb, A, x2=x2)
    want_pool = want_up = 0
    with torch.no_grad():
        out = None
        for i, name in enumerate(('encoder1', 'encoder2', 'encoder3')):
            blk = getattr(f, name)
            out = conv(blk['0'], cur, prev) if i == 0 else conv(blk['0'], out)
            hh, ww = out.shape[2], out.shape[3]
            want_pool += 0 if wino(blk['2'], hh, ww) and hh %% 2 == 0 and ww %% 2 == 0 else 1      # an odd map keeps its launch
            out = ops.maxpool2(conv(blk['2'], out))
        blocks = ('decoder1', 'decoder2', 'decoder3', 'flow')
        for i, name in enumerate(blocks[:3]):
            blk = getattr(f, name)
            out = ops.upsample(conv(blk['2'], conv(blk['0'], out)), 2, ops.UP_BILINEAR)
            want_up += 0 if wino(getattr(f, blocks[i + 1])['0'], out.shape[2], out.shape[3]) else 1
        head = f.flow['2']
        ref = ops.conv3x3_small(conv(f.flow['0'], out), head.weight.detach(), head.bias.detach(), ops.ACT_TANH24)
    torch.cuda.synchronize()
    got = (launches('maxpool2_kernel'), launches('upsample_kernel'))
    print((n, h, w), 'launches pool/up', got, 'expected', (want_pool, want_up), 'maxdiff', (flow - ref).abs().max().item())
    assert got == (want_pool, want_up), got
    assert flow.shape == ref.shape and torch.equal(flow, ref)
    return got

assert run(2, 16, 24) == (0, 0)       # forced: every pooled / up-sampled map has a Winograd neighbour
assert run(6, 70, 120) == (2, 0)      # the odd maps 35x60 and 17x30 keep their pool launch; several workgroups per layer
print('PLAN-OK')
"""


def test_fnet_plan_folds_pool_and_upsampling_into_winograd_neighbours():
    """FNet-only plans, 2 frame pairs of 16x24 (maps 16x24 ... 2x3) and 6 pairs of 70x120 (odd maps, several workgroups
    per layer: the encoder blocks pool in place, which the folded pool must not), with the Winograd form forced on every
    layer that has one (TG_CONV_WINO=1 is read once per process: a child): the flow equals the layers composed from
    separate ops bit for bit, and the only pool / up-sampling launches left are those of odd maps."""
    env = dict(os.environ, TG_CONV_WINO='1')
    r = subprocess.run([sys.executable, '-c', _PLAN_CHILD % (ROOT_DIR, GOLDEN_DIR)], env=env, timeout=600,
                       capture_output=True, text=True)
    assert r.returncode == 0 and 'PLAN-OK' in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
