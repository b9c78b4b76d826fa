"""GPU parity tests: the HIP path (through the C ABI) against
  (a) golden vectors produced by the upstream reference (tests/golden/*.npz),
  (b) the CPU oracle on seeded inputs,
  (c) size-independent properties at BASELINE.json's full sizes.

Tolerances (fp32, stated per test): single ops 1e-5 abs on O(1) data
(different summation order only); flow outputs 2e-4 (tanh*24 amplifies);
whole frames 1e-4 abs and |dPSNR| <= 1e-3 dB as BASELINE.json asks."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import os

from oracle import tecogan_oracle as O

ROOT_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_DIR = os.path.join(ROOT_DIR, 'tests', 'golden')
from procedural_weights import generator_state_dict, smooth_clip

T = torch.from_numpy


def dev(x):
    if isinstance(x, np.ndarray):
        x = T(x)
    return x.cuda().contiguous()


def err(a, b):
    a = a.detach().cpu().double() if torch.is_tensor(a) else T(np.asarray(a)).double()
    b = b.detach().cpu().double() if torch.is_tensor(b) else T(np.asarray(b)).double()
    return (a - b).abs().max().item()


def rs(seed, shape, lo=0.0, hi=1.0):
    return T(np.random.RandomState(seed).uniform(lo, hi, shape).astype(np.float32))


@pytest.fixture(scope='module')
def ops():
    import tecogan_pytorch_amd.ops as ops_
    from tecogan_pytorch_amd import _lib
    _lib.lib()
    return ops_


def make_net(deg, s):
    from tecogan_pytorch_amd.models.networks import FRNet
    net = FRNet(3, 3, 64, 10, deg, s)
    sd = generator_state_dict(scale=s, degradation=deg)
    net.load_state_dict(sd, strict=True)
    return net.cuda().eval(), sd


# ------------------------------------------------------------------ single ops
@pytest.mark.parametrize('case', ['', '_big', '_int', '_zero'])
def test_warp_vs_reference(golden, ops, case):
    g = golden('ops')
    x = g['warp_x']
    flow = np.zeros((2, 2, 17, 23), np.float32) if case == '_zero' else g['warp_flow' + case]
    out = ops.backward_warp(dev(x), dev(flow))
    assert err(out, g['warp_out' + case]) <= 5e-6
    # (zero flow is NOT a bit-exact identity in the reference either: positions go
    #  through the normalise / un-normalise round trip of grid_sample)


def test_warp_small_width(golden, ops):
    g = golden('ops')
    out = ops.backward_warp(dev(g['warp_x_small']), dev(g['warp_flow_small']))
    assert err(out, g['warp_out_small']) <= 5e-6


@pytest.mark.parametrize('s', [2, 4])
def test_space_to_depth_bit_exact(golden, ops, s):
    g = golden('ops')
    out = ops.space_to_depth(dev(g[f's2d{s}_x']), s)
    assert torch.equal(out.cpu(), T(g[f's2d{s}_out']))


@pytest.mark.parametrize('s', [2, 4])
def test_upsamplers_vs_reference(golden, ops, s):
    g = golden('ops')
    x = dev(g['up_x'])
    assert err(ops.upsample(x, s, ops.UP_BICUBIC), g[f'bicubic{s}_out']) <= 2e-6
    assert err(ops.upsample(x, s, ops.UP_BILINEAR), g[f'bilinear{s}_out']) <= 2e-6
    assert err(ops.upsample(x, s, ops.UP_BICUBIC, mul=float(s)), s * g[f'bicubic{s}_out']) <= 8e-6


def test_quantise_bit_exact(golden, ops):
    g = golden('ops')
    q = g['quant_x']
    n = q.size // 3 * 3
    x = dev(q[:n].reshape(3, 1, n // 3))
    out = ops.quantize_u8_hwc(x).cpu().numpy()          # (1, n/3, 3) hwc
    ref = g['quant_out'][:n].reshape(3, 1, n // 3).transpose(1, 2, 0)
    assert np.array_equal(out, ref)


def test_maxpool_floor_mode(ops):
    x = rs(5, (2, 5, 9, 13), -1, 1)
    out = ops.maxpool2(dev(x))
    ref = torch.nn.functional.max_pool2d(x, 2, 2)
    assert out.shape == ref.shape and torch.equal(out.cpu(), ref)


@pytest.mark.parametrize('shape', [(2, 5, 9, 12), (1, 3, 2, 4), (3, 4, 17, 40), (2, 3, 6, 16)])
def test_maxpool_vector_form_and_bilinear2x_vector_form(ops, shape):
    """w % 4 == 0: the 16-byte MaxPool2d(2, 2) kernel (exact: bit-identical to the CPU result, odd heights in
    floor mode); even w: the 2 x 4-patch bilinear x2 kernel against F.interpolate(align_corners=False)
    (tecogan_nets.py:49-61), incl. the clamped first / last rows and columns."""
    x = rs(6, shape, -1, 1)
    out = ops.maxpool2(dev(x))
    ref = torch.nn.functional.max_pool2d(x, 2, 2)
    assert out.shape == ref.shape and torch.equal(out.cpu(), ref)
    up = ops.upsample(dev(x), 2, ops.UP_BILINEAR, 3.0)
    ref = 3.0 * torch.nn.functional.interpolate(x, scale_factor=2, mode='bilinear', align_corners=False)
    assert up.shape == ref.shape and err(up, ref.numpy()) <= 4e-6


CONV_CASES = [
    # n, cin, cout, h, w, act, split(c1), residual
    (1, 64, 64, 22, 40, 1, None, False),
    (2, 64, 64, 13, 37, 0, None, True),       # ragged tile edges + residual
    (1, 6, 32, 22, 40, 2, 3, False),          # two-source cat, ocb 32, cin < chunk
    (1, 51, 64, 12, 20, 1, 3, False),         # SRNet conv_in: 3 + 48 channels
    (1, 32, 32, 9, 33, 2, None, False),
    (1, 128, 256, 5, 9, 2, None, False),      # FNet bottleneck: 4 oc groups, tiny map
    (1, 256, 128, 6, 10, 2, None, False),
    (1, 27, 64, 16, 16, 2, None, False),      # discriminator conv_in shape
    (1, 64, 64, 70, 96, 0, None, False),
    (3, 64, 64, 300, 260, 1, None, False),    # > 200k pixels: 4-row variant
    (1, 64, 48, 10, 34, 0, None, False),      # cout not a multiple of 32
]


@pytest.mark.parametrize('n,cin,cout,h,w,act,c1,use_res', CONV_CASES)
def test_conv3x3_mfma(ops, n, cin, cout, h, w, act, c1, use_res):
    """Asymmetric random weights: a transposed MFMA fragment mapping cannot pass."""
    import torch.nn.functional as F
    x = rs(1, (n, cin, h, w), -1, 1)
    wt = rs(2, (cout, cin, 3, 3), -1, 1) / (3.0 * cin ** 0.5)
    b = rs(3, (cout,), -0.5, 0.5)
    res = rs(4, (n, cout, h, w), -1, 1) if use_res else None
    ref = F.conv2d(x.double(), wt.double(), b.double(), padding=1)
    ref = {0: ref, 1: torch.relu(ref), 2: torch.where(ref >= 0, ref, ref * 0.2)}[act]
    if use_res:
        ref = ref + res.double()
    pk, ci_, co_, ocb = ops.pack_conv3x3(dev(wt))
    assert (ci_, co_) == (cin, cout)
    if c1:
        out = ops.conv3x3(dev(x[:, :c1]), pk, dev(b), cin, cout, ocb, act, x2=dev(x[:, c1:]),
                          res=None if res is None else dev(res))
    else:
        out = ops.conv3x3(dev(x), pk, dev(b), cin, cout, ocb, act,
                          res=None if res is None else dev(res))
    assert err(out, ref) <= 1e-5, err(out, ref)


WINO_CASES = [
    # n, cin, cout, h, w, act, split(c1), residual
    (1, 64, 64, 22, 40, 1, None, False),
    (2, 64, 64, 13, 37, 0, None, True),       # odd height and width: half tiles at both edges, scalar stores
    (1, 51, 64, 12, 20, 1, 3, False),         # SRNet conv_in: two sources, K padded 51 -> 64
    (1, 16, 64, 9, 33, 2, None, False),       # one K stage
    (1, 128, 128, 5, 9, 2, None, False),      # two output-channel groups, tiny map
    (1, 27, 64, 16, 16, 3, None, False),      # K padded 27 -> 32, tanh*24 epilogue
    (2, 64, 64, 134, 64, 0, None, True),      # 268 workgroups (the XCD-banded order starts at 512: the 134x320 tests)
    (1, 64, 48, 10, 34, 0, None, False),      # cout not a multiple of 16
    (1, 64, 64, 2, 2, 1, None, False),        # a single tile
]


@pytest.mark.parametrize('n,cin,cout,h,w,act,c1,use_res', WINO_CASES)
def test_conv3x3_winograd_form(ops, n, cin, cout, h, w, act, c1, use_res):
    """tg_conv3x3_wino_fwd (Winograd F(2x2,3x3) on the fp32 matrix cores) against an fp64
    convolution, same tolerance as the direct form."""
    import torch.nn.functional as F
    x = rs(1, (n, cin, h, w), -1, 1)
    wt = rs(2, (cout, cin, 3, 3), -1, 1) / (3.0 * cin ** 0.5)
    b = rs(3, (cout,), -0.5, 0.5)
    res = rs(4, (n, cout, h, w), -1, 1) if use_res else None
    ref = F.conv2d(x.double(), wt.double(), b.double(), padding=1)
    ref = {0: ref, 1: torch.relu(ref), 2: torch.where(ref >= 0, ref, ref * 0.2), 3: torch.tanh(ref) * 24}[act]
    if use_res:
        ref = ref + res.double()
    u = ops.pack_conv3x3_wino(dev(wt))
    kw = dict(res=None if res is None else dev(res))
    if c1:
        out = ops.conv3x3_wino(dev(x[:, :c1]), u, dev(b), cin, cout, act, x2=dev(x[:, c1:]), **kw)
    else:
        out = ops.conv3x3_wino(dev(x), u, dev(b), cin, cout, act, **kw)
    assert err(out, ref) <= (2e-5 if act == 3 else 1e-5), err(out, ref)


def test_conv3x3_winograd_data_gradient_and_relu_mask(ops):
    """transposed = 2 packing gives the data gradient of the layer; the ReLU-backward mask is
    applied in the epilogue (tg_conv3x3_fwd_masked semantics)."""
    import torch.nn.functional as F
    n, ci, co, h, w = 2, 32, 64, 11, 18
    x = rs(1, (n, ci, h, w), -1, 1).requires_grad_(True)
    wt = rs(2, (co, ci, 3, 3), -1, 1) / 10
    y = F.conv2d(torch.relu(x), wt, None, padding=1)
    dy = rs(3, tuple(y.shape), -1, 1)
    y.backward(dy)                                       # x.grad = dgrad(dy) masked by x > 0
    u = ops.pack_conv3x3_wino(dev(wt), transposed=2)
    got = ops.conv3x3_wino(dev(dy), u, None, co, ci, 0, mask=dev(torch.relu(x.detach())))
    assert err(got, x.grad) <= 1e-5, err(got, x.grad)


def test_winograd_full_size_properties(ops):
    """Size-independent properties at the BASELINE layer size (64 -> 64 at 134x320), where a CPU
    convolution is too slow for the suite: linearity in the input, equivariance under a shift by one
    2x2 tile, agreement with the direct MFMA form, run-to-run bit reproducibility."""
    g = torch.Generator().manual_seed(11)
    x1 = dev(torch.rand(1, 64, 134, 320, generator=g) - 0.5)
    x2 = dev(torch.rand(1, 64, 134, 320, generator=g) - 0.5)
    wt = dev((torch.rand(64, 64, 3, 3, generator=g) - 0.5) / 12)
    u = ops.pack_conv3x3_wino(wt)
    f = lambda x: ops.conv3x3_wino(x, u, None, 64, 64, 0)      # noqa: E731
    y1, y2 = f(x1), f(x2)
    y12 = f(ops_axpby(x1, 0.75, x2, -1.5))
    assert float((y12 - (0.75 * y1 - 1.5 * y2)).abs().max()) <= 2e-5
    xs = torch.zeros_like(x1)
    xs[:, :, 2:, 2:] = x1[:, :, :-2, :-2]                       # shift down / right by one tile
    ys = f(xs)
    # (the last row / column of ys sees zero padding where y1 saw data)
    assert torch.equal(ys[:, :, 4:-1, 4:-1], y1[:, :, 2:-3, 2:-3])
    pk = ops.pack_conv3x3(wt)
    yd = ops.conv3x3(x1, pk[0], None, 64, 64, pk[3], 0, ksplit=1)
    assert float((yd - y1).abs().max()) <= 2e-5
    assert torch.equal(f(x1), y1)


def ops_axpby(a, alpha, b, beta):
    return a * alpha + b * beta


@pytest.mark.parametrize('n,h,w', [(1, 26, 70), (2, 21, 37), (3, 134, 64)])
def test_winograd_chained_launch_equals_separate_launches(ops, n, h, w):
    """tg_conv3x3_wino_chain: SRNet's conv_in + residual blocks (two-source first layer, in-place
    residual sums, two ping-pong tensors) as ONE launch with per-tile flags must reproduce the
    separate launches bit for bit, launch after launch (stale data or a lost flag would show)."""
    g = torch.Generator().manual_seed(17)
    nb = 4
    lr, s2d = dev(torch.rand(n, 3, h, w, generator=g)), dev(torch.rand(n, 48, h, w, generator=g))
    ws = [dev(torch.randn(64, 51, 3, 3, generator=g) * 0.04)] + \
         [dev(torch.randn(64, 64, 3, 3, generator=g) * 0.03) for _ in range(2 * nb)]
    bs = [dev(torch.randn(64, generator=g) * 0.1) for _ in range(2 * nb + 1)]
    us = [ops.pack_conv3x3_wino(x) for x in ws]

    def make(A, B):
        layers = [dict(x=lr, x2=s2d, u=us[0], bias=bs[0], cin=51, act=1, y=A)]
        for b in range(nb):
            layers.append(dict(x=A, u=us[1 + 2 * b], bias=bs[1 + 2 * b], cin=64, act=1, y=B))
            layers.append(dict(x=B, u=us[2 + 2 * b], bias=bs[2 + 2 * b], cin=64, act=0, res=A, y=A))
        return layers
    A1, B1, A2, B2 = (torch.empty(n, 64, h, w, device='cuda') for _ in range(4))
    seq, chain = make(A1, B1), ops.WinoChain(make(A2, B2), n, 64, h, w)
    for it in range(8):
        lr.uniform_(); s2d.uniform_()
        for d in seq:
            ops.conv3x3_wino(d['x'], d['u'], d['bias'], d['cin'], 64, d['act'], x2=d.get('x2'), res=d.get('res'),
                             out=d['y'])
        chain.run()
        torch.cuda.synchronize()
        assert torch.equal(A1, A2) and torch.equal(B1, B2), it
    assert chain.bailouts() == 0


@pytest.mark.parametrize('h,w,nb,first', [(134, 320, 10, 'dual'), (26, 70, 4, 'dual'), (30, 50, 3, 'dual'), (8, 24, 2, 'dual'),
                                          (2, 2, 2, 'single'), (64, 96, 3, 'single'), (134, 320, 2, 'narrow')])
def test_winograd_resident_launch_equals_separate_launches(ops, h, w, nb, first):
    """tg_conv3x3_wino_resident (round 4): SRNet's conv_in + residual blocks of ONE frame on persistent,
    LDS-resident workgroups (8 x 24 pixel blocks, ring exchange through global memory, monotonic flags)
    must reproduce the per-layer Winograd launches BIT FOR BIT, launch after launch -- full blocks,
    partial blocks at the right / bottom border, a single block, the two-source 51-channel first
    layer, a 64-channel first layer read from global memory (the 2x plan's form) and a 15-channel one
    (4 K steps instead of 16)."""
    if not ops.WinoResident.supported(64, h, w):
        pytest.skip('frame does not fit one block per CU on this device')
    g = torch.Generator().manual_seed(23)
    cin0 = {'dual': 51, 'single': 64, 'narrow': 15}[first]
    c1 = {'dual': 3, 'single': 64, 'narrow': 3}[first]
    lr = dev(torch.rand(1, c1, h, w, generator=g))
    s2d = dev(torch.rand(1, cin0 - c1, h, w, generator=g)) if cin0 > c1 else None
    ws = [dev(torch.randn(64, cin0, 3, 3, generator=g) * 0.04)] + \
         [dev(torch.randn(64, 64, 3, 3, generator=g) * 0.03) for _ in range(2 * nb)]
    bs = [dev(torch.randn(64, generator=g) * 0.1) for _ in range(2 * nb + 1)]
    us = [ops.pack_conv3x3_wino(x) for x in ws]

    def make(A, B):
        layers = [dict(x=lr, x2=s2d, u=us[0], bias=bs[0], cin=cin0, act=1, y=A)]
        for b in range(nb):
            layers.append(dict(x=A, u=us[1 + 2 * b], bias=bs[1 + 2 * b], cin=64, act=1, y=B))
            layers.append(dict(x=B, u=us[2 + 2 * b], bias=bs[2 + 2 * b], cin=64, act=0, res=A, y=A))
        return layers
    A1, B1, A2, B2 = (torch.empty(1, 64, h, w, device='cuda') for _ in range(4))
    seq, res = make(A1, B1), ops.WinoResident(make(A2, B2), 64, h, w)
    for it in range(8):
        lr.uniform_(-1, 1)
        if s2d is not None:
            s2d.uniform_(-1, 1)
        A2.fill_(float('nan'))                   # the launch must write every pixel of its output
        for d in seq:
            ops.conv3x3_wino(d['x'], d['u'], d['bias'], d['cin'], 64, d['act'], x2=d.get('x2'), res=d.get('res'),
                             out=d['y'])
        res.run()
        torch.cuda.synchronize()
        assert res.bailouts() == 0
        assert torch.equal(A1, A2), (it, (A1 - A2).abs().max().item(), int((A1 != A2).sum()))


@pytest.mark.parametrize('h,w,nb', [(134, 320, 2), (26, 70, 1), (8, 24, 1), (30, 50, 2), (2, 2, 1)])
def test_winograd_resident_launch_with_transposed_conv_tail(ops, h, w, nb):
    """tg_conv3x3_wino_resident_ct: SRNet's first ConvTranspose2d(64, 64, 3, 2, 1, 1) + ReLU (tecogan_nets.py:119-126)
    as the tail of the resident launch, against the per-layer launches followed by the stand-alone transposed-conv
    kernel and against torch's CPU conv_transpose2d (fp64): 3e-6 relative to the output scale (fp32 products of
    K = 576, another summation order), full / partial / single blocks, every output pixel written."""
    if not ops.WinoResident.supported(64, h, w):
        pytest.skip('frame does not fit one block per CU on this device')
    g = torch.Generator().manual_seed(29)
    lr = dev(torch.rand(1, 3, h, w, generator=g))
    s2d = dev(torch.rand(1, 48, h, w, generator=g))
    ws = [dev(torch.randn(64, 51, 3, 3, generator=g) * 0.04)] + \
         [dev(torch.randn(64, 64, 3, 3, generator=g) * 0.03) for _ in range(2 * nb)]
    bs = [dev(torch.randn(64, generator=g) * 0.1) for _ in range(2 * nb + 1)]
    us = [ops.pack_conv3x3_wino(x) for x in ws]
    wt = torch.randn(64, 64, 3, 3, generator=g) * 0.05          # (cin, cout, 3, 3)
    bt = torch.randn(64, generator=g) * 0.1

    def make(A, B):
        layers = [dict(x=lr, x2=s2d, u=us[0], bias=bs[0], cin=51, act=1, y=A)]
        for b in range(nb):
            layers.append(dict(x=A, u=us[1 + 2 * b], bias=bs[1 + 2 * b], cin=64, act=1, y=B))
            layers.append(dict(x=B, u=us[2 + 2 * b], bias=bs[2 + 2 * b], cin=64, act=0, res=A, y=A))
        return layers
    A1, B1, A2, B2 = (torch.empty(1, 64, h, w, device='cuda') for _ in range(4))
    seq, res = make(A1, B1), ops.WinoResident(make(A2, B2), 64, h, w)
    ct = dict(u=ops.pack_wres_convt(dev(wt)), bias=dev(bt), y=torch.empty(1, 64, 2 * h, 2 * w, device='cuda'), act=1)
    pk, _, _, _ = ops.pack_conv3x3(dev(wt), transposed=True)
    for it in range(3):
        lr.uniform_(-1, 1); s2d.uniform_(-1, 1)
        ct['y'].fill_(float('nan'))
        for d in seq:
            ops.conv3x3_wino(d['x'], d['u'], d['bias'], d['cin'], 64, d['act'], x2=d.get('x2'), res=d.get('res'), out=d['y'])
        ref_gpu = ops.convt3x3s2(A1, pk, dev(bt), 64, 1)
        res.run(convt=ct)
        torch.cuda.synchronize()
        assert res.bailouts() == 0
        ref = torch.relu(torch.nn.functional.conv_transpose2d(A1.cpu().double(), wt.double(), bt.double(), 2, 1, 1))
        scale = ref.abs().max().item()
        assert not torch.isnan(ct['y']).any()
        assert (ct['y'].cpu().double() - ref).abs().max().item() <= 3e-6 * scale, it
        assert (ct['y'] - ref_gpu).abs().max().item() <= 3e-6 * scale, it
    res.run()                                     # and the launch without the tail still writes the body's output
    torch.cuda.synchronize()
    assert torch.equal(A1, A2)


def test_winograd_resident_rejects_foreign_buffer_patterns(ops):
    """The resident launch keeps the intermediate tensors in LDS, so it insists on the chain pattern of
    the reference's SRNet (tecogan_nets.py:85-100): anything else is refused, not silently mis-computed."""
    from tecogan_pytorch_amd import _lib
    h, w = 16, 48
    if not ops.WinoResident.supported(64, h, w):
        pytest.skip('not supported on this device')
    x, A, B, C = (torch.zeros(1, 64, h, w, device='cuda') for _ in range(4))
    u = ops.pack_conv3x3_wino(torch.zeros(64, 64, 3, 3, device='cuda'))
    b = torch.zeros(64, device='cuda')
    ok = [dict(x=x, u=u, bias=b, cin=64, act=1, y=A), dict(x=A, u=u, bias=b, cin=64, act=0, res=x, y=B)]
    ops.WinoResident(ok, 64, h, w).run()
    bad_dep = [dict(x=x, u=u, bias=b, cin=64, act=1, y=A), dict(x=C, u=u, bias=b, cin=64, act=0, y=B)]
    bad_res = [dict(x=x, u=u, bias=b, cin=64, act=1, y=A), dict(x=A, u=u, bias=b, cin=64, act=0, res=C, y=B)]
    no_bias = [dict(x=x, u=u, cin=64, act=1, y=A)]
    for layers in (bad_dep, bad_res, no_bias):
        with pytest.raises(_lib.TecoganHipError):
            ops.WinoResident(layers, 64, h, w).run()
    assert not ops.WinoResident.supported(64, 15, 48) and not ops.WinoResident.supported(32, 16, 48)
    assert not ops.WinoResident.supported(64, 16, 48, n=2) and not ops.WinoResident.supported(64, 268, 640)
    torch.cuda.synchronize()


def test_winograd_chain_numerics_at_trained_activation_scale(ops):
    """SRNet's 20 residual-block layers at the activation magnitudes of a TRAINED model (|x| grows
    from ~10^2 to ~10^3 along the residual chain; the procedural parity weights stay O(1)): the
    Winograd form -- layer by layer and as the chained launch -- must be as close to an fp64 chain
    as the direct fp32-MFMA form is (the transforms only add, but they add BEFORE the products)."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(0)
    nf, nb, h, w = 64, 10, 66, 80
    x = 100.0 * torch.rand(1, nf, h, w, generator=g)
    ws = [torch.randn(nf, nf, 3, 3, generator=g) * (2.0 / (nf * 9)) ** 0.5 for _ in range(2 * nb)]
    a = x.double()
    for b in range(nb):
        a = a + F.conv2d(torch.relu(F.conv2d(a, ws[2 * b].double(), padding=1)), ws[2 * b + 1].double(), padding=1)
    ref = a
    assert 50 < ref.abs().mean() and 500 < ref.abs().max() < 1e5, (ref.abs().mean(), ref.abs().max())
    wd = [dev(t) for t in ws]
    us = [ops.pack_conv3x3_wino(t) for t in wd]
    pk = [ops.pack_conv3x3(t) for t in wd]

    def run(conv):
        A = dev(x).clone()
        for b in range(nb):
            B = conv(A, 2 * b, 1, None)
            A = conv(B, 2 * b + 1, 0, A)
        return A
    direct = run(lambda t, i, act, res: ops.conv3x3(t, pk[i][0], None, nf, nf, pk[i][3], act, res=res, ksplit=1))
    wino = run(lambda t, i, act, res: ops.conv3x3_wino(t, us[i], None, nf, nf, act, res=res))
    A, B = dev(x).clone(), torch.empty(1, nf, h, w, device='cuda')
    layers = []
    for b in range(nb):
        layers.append(dict(x=A, u=us[2 * b], cin=nf, act=1, y=B))
        layers.append(dict(x=B, u=us[2 * b + 1], cin=nf, act=0, res=A, y=A))
    chain = ops.WinoChain(layers, 1, nf, h, w)
    chain.run()
    torch.cuda.synchronize()
    assert chain.bailouts() == 0
    A3, B3 = dev(x).clone(), torch.empty(1, nf, h, w, device='cuda')
    bz = torch.zeros(nf, device='cuda')
    layers3 = []
    for b in range(nb):
        layers3.append(dict(x=A3, u=us[2 * b], bias=bz, cin=nf, act=1, y=B3))
        layers3.append(dict(x=B3, u=us[2 * b + 1], bias=bz, cin=nf, act=0, res=A3, y=A3))
    if ops.WinoResident.supported(nf, h, w):
        resident = ops.WinoResident(layers3, nf, h, w)
        resident.run()
        torch.cuda.synchronize()
        assert resident.bailouts() == 0
        assert torch.equal(wino, A3)                              # resident launch == separate launches
    e = {k: (v.double().cpu() - ref).abs() for k, v in (('direct', direct), ('wino', wino), ('chain', A))}
    scale = ref.abs().max().item()
    for k in e:
        assert e[k].max().item() <= 2e-6 * scale, (k, e[k].max().item(), scale)      # fp32 through 20 layers
    assert torch.equal(wino, A)                                   # chained launch == separate launches
    # no worse than the direct form (max and mean error, 25 % slack for run-to-run tile-order noise)
    assert e['wino'].max() <= 1.25 * e['direct'].max() + 1e-7 * scale, (e['wino'].max(), e['direct'].max())
    assert e['wino'].mean() <= 1.25 * e['direct'].mean() + 1e-8 * scale, (e['wino'].mean(), e['direct'].mean())


def test_plan_with_chained_srnet_launch(tmp_path):
    """The frame plan with SRNet as one chained launch (TG_WINO_CHAIN=1) against the plan with one launch
    per layer: same kernels, so the frames must be bit-identical.  (The switches are read once per
    process: two subprocesses.)"""
    import subprocess
    import sys
    script = (
        "import sys, torch; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "from tests.test_hip_parity import make_net, smooth_clip\n"
        "net, _ = make_net('BD', 4)\n"
        "import numpy as np\n"
        "x = torch.from_numpy(np.stack([smooth_clip(6, 3, 26, 40, seed=5), smooth_clip(6, 3, 26, 40, seed=6)])).cuda()\n"
        "y = net.infer_sequence(x, torch.device('cuda'), return_device_tensor=True)\n"
        "torch.save(y.cpu(), sys.argv[1])\n" % (ROOT_DIR, GOLDEN_DIR))
    outs = []
    for chain in ('0', '1'):
        env = dict(os.environ, TG_CONV_WINO='1', TG_WINO_CHAIN=chain)
        out = str(tmp_path / ('y%s.pt' % chain))
        subprocess.run([sys.executable, '-c', script, out], check=True, env=env, timeout=600)
        outs.append(torch.load(out))
    assert outs[0].shape == outs[1].shape and torch.equal(outs[0], outs[1])


def test_plan_with_resident_srnet_launch(tmp_path):
    """The frame plan with SRNet's body as the LDS-resident launch (the default for one 134x320-class frame)
    against the plan with one launch per layer (TG_WINO_RES=0): bit-identical uint8 AND fp32 frames of a
    recurrent clip, serial and pipelined, and the plan statistics name the class.  (The switch is read
    once per process: two subprocesses.)"""
    import subprocess
    import sys
    script = (
        "import sys, ctypes, torch; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "from tests.test_hip_parity import make_net, smooth_clip\n"
        "from tecogan_pytorch_amd import _lib\n"
        "net, _ = make_net('BD', 4)\n"
        "dev = torch.device('cuda', 0)\n"
        "x = smooth_clip(7, 3, 70, 120, seed=5).cuda()\n"
        "y0 = net.infer_sequence(x, dev, return_device_tensor=True, pipeline=False)\n"
        "y1 = net.infer_sequence(x, dev, return_device_tensor=True, pipeline=True)\n"
        "z = torch.rand(1, 3, 280, 480, generator=torch.Generator().manual_seed(3)).cuda()\n"
        "f = net.step(x[1:2], x[0:1], z)\n"
        "torch.cuda.synchronize(); net.check_faults()\n"
        "plan = net._get_plan(1, 70, 120, dev)\n"
        "lib = _lib.lib()\n"
        "names = [lib.tg_frnet_kind_name(k).decode() for k in range(lib.tg_frnet_plan_kinds())]\n"
        "nl = ctypes.c_int()\n"
        "_lib.check(lib.tg_frnet_plan_kind_stats(plan.handle, names.index('conv3x3_wino_resident_kernel'), ctypes.byref(nl), None, None), 'ks')\n"
        "torch.save(dict(y0=y0.cpu(), y1=y1.cpu(), f=f.cpu(), resident=nl.value, state=plan.chain_state()), sys.argv[1])\n"
        % (ROOT_DIR, GOLDEN_DIR))
    outs = []
    for flag, tail in (('0', '0'), ('1', '0'), ('1', '1')):
        env = dict(os.environ, TG_WINO_RES=flag, TG_CONV_WINO='1', TG_WINO_RES_CT=tail)
        out = str(tmp_path / ('y%s%s.pt' % (flag, tail)))
        subprocess.run([sys.executable, '-c', script, out], check=True, env=env, timeout=600)
        outs.append(torch.load(out))
    assert outs[0]['resident'] == 0 and outs[1]['resident'] == 1 and outs[2]['resident'] == 1
    assert outs[1]['state'] == (0, True) and outs[2]['state'] == (0, True), (outs[1]['state'], outs[2]['state'])
    for k in ('y0', 'y1', 'f'):
        assert outs[0][k].shape == outs[1][k].shape and torch.equal(outs[0][k], outs[1][k]), k
    # the default: the first transposed conv as the launch's tail (direct fp32 products in another summation order
    # than the stand-alone kernel): fp32 frame to 2e-5, uint8 frames to one level on <= 0.2 % of the pixels
    assert (outs[2]['f'] - outs[0]['f']).abs().max().item() <= 2e-5
    for k in ('y0', 'y1'):
        d = (outs[2][k].to(torch.int16) - outs[0][k].to(torch.int16)).abs()
        assert d.max().item() <= 1 and (d > 0).float().mean().item() <= 2e-3, (k, d.max().item())


def test_resident_launch_fault_surfaces_and_falls_back(tmp_path):
    """Fail-safe of the LDS-resident SRNet launch: with fault injection (negative poll limit) the error
    surfaces on the host-output path / on the next call, the plan then runs one launch per layer and
    reproduces a never-resident run bit for bit."""
    import subprocess
    import sys
    script = (
        "import sys, torch; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import numpy as np\n"
        "from tests.test_hip_parity import make_net, smooth_clip\n"
        "from tecogan_pytorch_amd import _lib\n"
        "E = _lib.TecoganHipError\n"
        "dev = torch.device('cuda', 0)\n"
        "x = smooth_clip(5, 3, 40, 72, seed=5).cuda()\n"
        "def fresh(inject):\n"
        "    net, _ = make_net('BD', 4)\n"
        "    plan = net._get_plan(1, 40, 72, dev)\n"
        "    assert plan.chain_state() == (0, True), plan.chain_state()\n"
        "    if inject: _lib.check(_lib.lib().tg_frnet_plan_set_chain_poll_limit(plan.handle, -1), 'limit')\n"
        "    return net, plan\n"
        "def raises(fn):\n"
        "    try: fn()\n"
        "    except E as e: return 'timed out' in str(e)\n"
        "    return False\n"
        "ref_net, _ = fresh(False)\n"
        "ref = ref_net.infer_sequence(x, dev)\n"
        "net, plan = fresh(True)\n"
        "assert raises(lambda: net.infer_sequence(x, dev, on_fault='raise')), 'no error on the host-output path'\n"
        "torch.cuda.synchronize()\n"
        "f, active = plan.chain_state(); assert f > 0 and not active, (f, active)\n"
        "assert np.array_equal(net.infer_sequence(x, dev), ref), 'fallback differs'\n"
        "# the default (on_fault='rerun'): the caller gets the correct clip and a warning, not an error (ADVICE r4)\n"
        "import warnings\n"
        "net, plan = fresh(True)\n"
        "with warnings.catch_warnings(record=True) as wl:\n"
        "    warnings.simplefilter('always')\n"
        "    y = net.infer_sequence(x, dev)\n"
        "assert any('computed again' in str(w_.message) for w_ in wl), [str(w_.message) for w_ in wl]\n"
        "assert np.array_equal(y, ref), 'rerun differs'\n"
        "f, active = plan.chain_state(); assert f > 0 and not active, (f, active)\n"
        "net, plan = fresh(True)\n"
        "y = net.infer_sequence(x[:1], dev, return_device_tensor=True); torch.cuda.synchronize()\n"
        "assert raises(lambda: net.infer_sequence(x[:1], dev, return_device_tensor=True)), 'next call silent'\n"
        "print('FAILSAFE-OK')\n" % (ROOT_DIR, GOLDEN_DIR))
    # (TG_WINO_RES_CT=0: the healthy reference run keeps the first transposed conv a launch of its own, as the
    # fallen-back plan does -- the comparison is about the fallback machinery, bit for bit)
    env = dict(os.environ, TG_WINO_RES='1', TG_CONV_WINO='1', TG_WINO_RES_CT='0')
    r = subprocess.run([sys.executable, '-c', script], env=env, timeout=600, capture_output=True, text=True)
    assert r.returncode == 0 and 'FAILSAFE-OK' in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


@pytest.mark.parametrize('kind,k,h,w', [('resident', 1, 40, 72), ('chain', 2, 26, 40)])
def test_resident_launch_recovers_from_a_transient_fault(tmp_path, kind, k, h, w):
    """(kind 'chain': the same protocol for the chained Winograd launch of a 2-clip plan.)
    VERDICT r5 item 7 / ADVICE r4 item 3: ONE injected fault (a transient co-tenant) must not cost the one-launch
    body for the life of the process.  The plan falls back to one launch per layer, counts clean frames, arms the
    resident launch again after the back-off (here 6 frames instead of the default 64), and a second fault doubles
    the wait.  Frames are bit-identical on either path (TG_WINO_RES_CT=0: the first transposed conv a launch of its
    own on both)."""
    import subprocess
    import sys
    script = (
        "import sys, torch, warnings; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import numpy as np\n"
        "from tests.test_hip_parity import make_net, smooth_clip\n"
        "from tecogan_pytorch_amd import _lib\n"
        "dev = torch.device('cuda', 0)\n"
        "K, H, W = %d, %d, %d\n"
        "x = smooth_clip(5, 3, H, W, seed=5).cuda() if K == 1 else torch.from_numpy(np.stack([smooth_clip(5, 3, H, W, seed=5 + i) for i in range(K)])).cuda()\n"
        "net, _ = make_net('BD', 4)\n"
        "plan = net._get_plan(K, H, W, dev)\n"
        "plan.set_chain_rearm(6)\n"
        "limit = lambda v: _lib.check(_lib.lib().tg_frnet_plan_set_chain_poll_limit(plan.handle, v), 'limit')\n"
        "ref = net.infer_sequence(x, dev)                       # healthy: resident body\n"
        "assert plan.chain_state() == (0, True) and plan.rearm_state() == (0, 0)\n"
        "def faulted_clip():\n"
        "    limit(-1)\n"
        "    with warnings.catch_warnings(record=True) as wl:\n"
        "        warnings.simplefilter('always')\n"
        "        y = net.infer_sequence(x, dev)                  # faults, is computed again on the fallback (5 clean frames)\n"
        "    limit(1 << 21)\n"
        "    assert any('computed again' in str(w_.message) for w_ in wl)\n"
        "    return y\n"
        "y = faulted_clip()\n"
        "assert np.array_equal(y, ref), 'rerun differs'\n"
        "f1, active = plan.chain_state(); assert f1 > 0 and not active, (f1, active)\n"
        "assert plan.rearm_state() == (0, 6), plan.rearm_state()\n"
        "y = net.infer_sequence(x, dev)                          # frames 6..10 on the fallback: the back-off passes inside this clip\n"
        "assert np.array_equal(y, ref), 'fallback differs'\n"
        "y = net.infer_sequence(x, dev)\n"
        "assert np.array_equal(y, ref), 're-armed body differs'\n"
        "f, active = plan.chain_state(); assert f == f1 and active, ('not re-armed', f, f1, active)\n"
        "assert plan.rearm_state() == (1, 6), plan.rearm_state()\n"
        "# the re-armed body really is the one launch again: a second injected fault is seen, and doubles the wait\n"
        "y = faulted_clip()\n"
        "assert np.array_equal(y, ref)\n"
        "f2, active = plan.chain_state(); assert f2 > f1 and not active, (f2, f1, active)\n"
        "assert plan.rearm_state() == (1, 12), plan.rearm_state()\n"
        "for _ in range(2): assert np.array_equal(net.infer_sequence(x, dev), ref)     # 5 (rerun) + 10 clean frames >= 12\n"
        "assert np.array_equal(net.infer_sequence(x, dev), ref)\n"
        "assert plan.chain_state() == (f2, True) and plan.rearm_state() == (2, 12), (plan.chain_state(), plan.rearm_state())\n"
        "# first_after_frames = 0: the round-5 behaviour, off for good\n"
        "plan.set_chain_rearm(0)\n"
        "y = faulted_clip()\n"
        "for _ in range(8): assert np.array_equal(net.infer_sequence(x, dev), ref)\n"
        "assert not plan.chain_state()[1] and plan.rearm_state()[0] == 2\n"
        "print('REARM-OK')\n" % (ROOT_DIR, GOLDEN_DIR, k, h, w))
    env = dict(os.environ, TG_WINO_RES='1', TG_CONV_WINO='1', TG_WINO_RES_CT='0') if kind == 'resident' else \
        dict(os.environ, TG_CONV_WINO='1', TG_WINO_CHAIN='1')
    r = subprocess.run([sys.executable, '-c', script], env=env, timeout=600, capture_output=True, text=True)
    assert r.returncode == 0 and 'REARM-OK' in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_chained_launch_fault_surfaces_on_every_path(tmp_path):
    """Fail-safe of the chained SRNet launch: with fault injection (negative poll limit: every waiting
    workgroup gives up at once) the error must surface (a) at infer_sequence's host-output exit,
    (b) on the call after a `return_device_tensor=True` clip and in check_faults() after the caller's
    sync, (c) on the step() after a faulted step() -- and after the report the plan must have fallen
    back to one launch per layer and produce the frames of a never-chained run, bit for bit."""
    import subprocess
    import sys
    script = (
        "import sys, torch; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import numpy as np\n"
        "from tests.test_hip_parity import make_net, smooth_clip\n"
        "from tecogan_pytorch_amd import _lib\n"
        "E = _lib.TecoganHipError\n"
        "dev = torch.device('cuda', 0)\n"
        "x = torch.from_numpy(np.stack([smooth_clip(5, 3, 26, 40, seed=5), smooth_clip(5, 3, 26, 40, seed=6)])).cuda()\n"
        "def fresh(inject):\n"
        "    net, _ = make_net('BD', 4)\n"
        "    plan = net._get_plan(2, 26, 40, dev)\n"
        "    assert plan.chain_state() == (0, True), plan.chain_state()\n"
        "    if inject: _lib.check(_lib.lib().tg_frnet_plan_set_chain_poll_limit(plan.handle, -1), 'limit')\n"
        "    return net, plan\n"
        "def raises(fn):\n"
        "    try: fn()\n"
        "    except E as e: return 'timed out' in str(e)\n"
        "    return False\n"
        "ref_net, _ = fresh(False)\n"
        "ref = ref_net.infer_sequence(x, dev)\n"
        "def synced(fn):\n"
        "    def go():\n"
        "        r = fn(); torch.cuda.synchronize(); net.check_faults(); return r\n"
        "    return go\n"
        "# (a) host-output exit (the entry check of a later frame's call may fire first: same error)\n"
        "net, plan = fresh(True)\n"
        "assert raises(lambda: net.infer_sequence(x, dev, on_fault='raise')), 'a: no error on the host-output path'\n"
        "torch.cuda.synchronize()\n"
        "f, active = plan.chain_state(); assert f > 0 and not active, (f, active)\n"
        "assert np.array_equal(net.infer_sequence(x, dev), ref), 'a: fallback differs'\n"
        "# (b) device-tensor exit: nothing is synchronised inside -> the caller's check after its own sync\n"
        "net, plan = fresh(True)\n"
        "assert raises(synced(lambda: net.infer_sequence(x, dev, return_device_tensor=True))), 'b: check_faults silent'\n"
        "torch.cuda.synchronize()\n"
        "y = synced(lambda: net.infer_sequence(x, dev, return_device_tensor=True))()\n"
        "assert np.array_equal(y.cpu().numpy(), ref), 'b: fallback differs'\n"
        "# (b') ONE chained launch (a 1-frame clip), then a sync: the NEXT call must refuse at its entry\n"
        "net, plan = fresh(True)\n"
        "y = net.infer_sequence(x[:, :1], dev, return_device_tensor=True); torch.cuda.synchronize()\n"
        "assert raises(lambda: net.infer_sequence(x[:, :1], dev, return_device_tensor=True)), 'b2: next call silent'\n"
        "# (c) step() with n = 2: same, through FRNet.step\n"
        "net, plan = fresh(True)\n"
        "z = torch.zeros(2, 3, 104, 160, device='cuda')\n"
        "o = net.step(x[:, 1], x[:, 0], z); torch.cuda.synchronize()\n"
        "assert raises(lambda: net.step(x[:, 1], x[:, 0], z)), 'c: next step silent'\n"
        "o2 = synced(lambda: net.step(x[:, 1], x[:, 0], z))()\n"
        "o3 = ref_net.step(x[:, 1], x[:, 0], z); torch.cuda.synchronize(); ref_net.check_faults()\n"
        "assert torch.equal(o2, o3), 'c: fallback differs'\n"
        "print('FAILSAFE-OK')\n" % (ROOT_DIR, GOLDEN_DIR))
    env = dict(os.environ, TG_CONV_WINO='1', TG_WINO_CHAIN='1')
    r = subprocess.run([sys.executable, '-c', script], env=env, timeout=600, capture_output=True, text=True)
    assert r.returncode == 0 and 'FAILSAFE-OK' in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_winograd_rule_and_plan_use(ops):
    """The frame plan runs SRNet's full-resolution layers in the Winograd form (and says so in its
    per-class statistics); tiny frames stay on the direct kernels."""
    from tecogan_pytorch_amd import _lib
    lib = _lib.lib()
    assert lib.tg_conv3x3_prefers_wino(1, 64, 64, 134, 320) == 1
    assert lib.tg_conv3x3_prefers_wino(1, 64, 64, 32, 32) == 0 and lib.tg_conv3x3_prefers_wino(36, 32, 64, 16, 16) == 1
    assert lib.tg_conv3x3_prefers_wino(1, 64, 64, 67, 160) == 1
    assert lib.tg_conv3x3_prefers_wino(1, 6, 64, 134, 320) == 0 and lib.tg_conv3x3_prefers_wino(1, 64, 32, 134, 320) == 0
    net, _ = make_net('BD', 4)
    plan = net._get_plan(1, 134, 320, torch.device('cuda'))
    import ctypes
    names = [lib.tg_frnet_kind_name(k).decode() for k in range(lib.tg_frnet_plan_kinds())]
    nl, nc = ctypes.c_int(), ctypes.c_int()
    _lib.check(lib.tg_frnet_plan_kind_stats(plan.handle, names.index('conv3x3_wino_kernel'), ctypes.byref(nl),
                                            None, None), 'kind_stats')
    _lib.check(lib.tg_frnet_plan_kind_stats(plan.handle, names.index('conv3x3_wino_chain_kernel'),
                                            ctypes.byref(nc), None, None), 'kind_stats')
    nr = ctypes.c_int()
    _lib.check(lib.tg_frnet_plan_kind_stats(plan.handle, names.index('conv3x3_wino_resident_kernel'),
                                            ctypes.byref(nr), None, None), 'kind_stats')
    # SRNet conv_in + 10 residual blocks (21 launches, or one chained launch under TG_WINO_CHAIN=1, or --
    # the default for one 134x320 frame since round 4 -- one LDS-resident launch) and FNet's four 67x160 layers
    if 'TG_CONV_WINO' not in os.environ:        # (a forced rule changes the mix)
        assert nl.value + 21 * (nc.value + nr.value) == 25 and nc.value + nr.value in (0, 1)
        if 'TG_WINO_RES' not in os.environ and 'TG_WINO_CHAIN' not in os.environ:
            assert nr.value == 1


@pytest.mark.parametrize('n,cin,cout,h,w,ks,pool', [
    (1, 256, 256, 16, 40, 8, False), (1, 128, 128, 33, 80, 4, True), (2, 64, 64, 9, 21, 2, True),
    (1, 128, 256, 16, 40, None, False), (1, 64, 128, 33, 80, None, True)])
def test_conv3x3_splitk(ops, n, cin, cout, h, w, ks, pool):
    """Deterministic split-K path (FNet middle layers) incl. the fused MaxPool2d."""
    import torch.nn.functional as F
    x = rs(1, (n, cin, h, w), -1, 1)
    wt = rs(2, (cout, cin, 3, 3), -1, 1) / (3.0 * cin ** 0.5)
    b = rs(3, (cout,), -0.5, 0.5)
    ref = F.conv2d(x.double(), wt.double(), b.double(), padding=1)
    ref = torch.where(ref >= 0, ref, ref * 0.2)
    if pool:
        ref = F.max_pool2d(ref, 2, 2)
    pk, _, _, ocb = ops.pack_conv3x3(dev(wt))
    out = ops.conv3x3(dev(x), pk, dev(b), cin, cout, ocb, 2, pool=pool, ksplit=ks)
    assert out.shape == ref.shape and err(out, ref) <= 1e-5, err(out, ref)
    out2 = ops.conv3x3(dev(x), pk, dev(b), cin, cout, ocb, 2, pool=pool, ksplit=ks)
    assert torch.equal(out, out2)          # fixed summation order: bit-reproducible


def test_conv3x3_inplace_residual(ops):
    """The resblock tail writes `conv(t) + x` over x (plan does this)."""
    import torch.nn.functional as F
    x = rs(1, (1, 64, 20, 40), -1, 1)
    t = rs(5, (1, 64, 20, 40), -1, 1)
    wt = rs(2, (64, 64, 3, 3), -1, 1) / 24.0
    b = rs(3, (64,), -0.5, 0.5)
    ref = F.conv2d(t.double(), wt.double(), b.double(), padding=1) + x.double()
    pk, _, _, ocb = ops.pack_conv3x3(dev(wt))
    xd = dev(x)
    ops.conv3x3(dev(t), pk, dev(b), 64, 64, ocb, 0, res=xd, out=xd)
    assert err(xd, ref) <= 1e-5


@pytest.mark.parametrize('n,cin,cout,h,w', [(1, 64, 64, 12, 20), (2, 64, 64, 7, 35),
                                            (1, 64, 64, 33, 64), (1, 16, 40, 5, 6),
                                            # > 256 one-row tiles: the chunk-by-chunk kernel (2- and 4-row workgroups)
                                            (2, 64, 64, 70, 66), (3, 64, 64, 130, 40), (1, 72, 64, 9, 33),
                                            # the training frames: one-shot kernel
                                            (2, 64, 64, 32, 32), (2, 64, 64, 64, 64), (2, 51, 37, 11, 70)])
def test_convt3x3s2_mfma(ops, n, cin, cout, h, w):
    import torch.nn.functional as F
    x = rs(1, (n, cin, h, w), -1, 1)
    wt = rs(2, (cin, cout, 3, 3), -1, 1) / (1.5 * cin ** 0.5)
    b = rs(3, (cout,), -0.5, 0.5)
    ref = torch.relu(F.conv_transpose2d(x.double(), wt.double(), b.double(), stride=2, padding=1,
                                        output_padding=1))
    pk, ci_, co_, ocb = ops.pack_conv3x3(dev(wt), transposed=True)
    assert (ci_, co_, ocb) == (cin, cout, 64)
    out = ops.convt3x3s2(dev(x), pk, dev(b), cout, 1)
    assert out.shape == ref.shape and err(out, ref) <= 1e-5, err(out, ref)


@pytest.mark.parametrize('n,cin,cout,cz,h,w', [(1, 64, 64, 3, 12, 20), (2, 64, 64, 3, 7, 35), (1, 64, 64, 3, 33, 64),
                                               (1, 40, 48, 2, 9, 33), (2, 64, 64, 1, 21, 70), (1, 64, 64, 3, 70, 130)])
def test_convt_z_forms_are_bit_identical_write_only_their_planes_and_match_the_composition(ops, n, cin, cout, cz, h, w):
    """tg_convt3x3s2_z_fwd_form: the last up-sampling layer + the output conv's channel contraction (Z mode,
    tecogan_nets.py:119-131).  The tiled form must be the reference composition, plane[tap * cz + o] =
    sum_c Wout[o, c, tap] * relu(convT(x))[c], on ragged shapes (w not a multiple of 32, odd h, n = 2, fewer channels),
    and every form a caller can ask for (0 one launch, 3 split tail -- one launch where the image has no whole round --,
    -1 the rule), three launches in a row into a pre-filled buffer, must equal it BIT FOR BIT and leave the planes
    behind 9 * cz untouched."""
    import torch.nn.functional as F
    x = rs(1, (n, cin, h, w), -1, 1)
    wt = rs(2, (cin, cout, 3, 3), -1, 1) / (1.5 * cin ** 0.5)
    b = rs(3, (cout,), -0.5, 0.5)
    wo = rs(4, (cz, cout, 3, 3), -1, 1) / (3.0 * cout ** 0.5)
    up = torch.relu(F.conv_transpose2d(x.double(), wt.double(), b.double(), stride=2, padding=1, output_padding=1))
    ref = torch.einsum('octk,nchw->ntkohw', wo.double().reshape(cz, cout, 3, 3), up).reshape(n, 9 * cz, 2 * h, 2 * w)
    pk, _, _, _ = ops.pack_conv3x3(dev(wt), transposed=True)
    wz = ops.convt_pack_wz(dev(wo))
    xd, bd = dev(x), dev(b)
    tiled = ops.convt3x3s2_z(xd, pk, bd, wz, cz, cout, act=1, form=0)
    assert err(tiled[:, :9 * cz], ref) <= 1e-5, err(tiled[:, :9 * cz], ref)
    for form in (0, 3, -1):
        out = torch.full((n, 32, 2 * h, 2 * w), 7.0, device='cuda')
        ops.convt3x3s2_z(xd, pk, bd, wz, cz, cout, act=1, form=form, out=out)
        assert torch.equal(out[:, :9 * cz], tiled[:, :9 * cz]), (form, (out[:, :9 * cz] - tiled[:, :9 * cz]).abs().max().item())
        assert bool((out[:, 9 * cz:] == 7.0).all()), f'form {form} wrote outside its planes'
    auto = ops.convt3x3s2_z(xd, pk, bd, wz, cz, cout, act=1)
    assert torch.equal(auto[:, :9 * cz], tiled[:, :9 * cz])


def test_convt_z_split_tail_is_bit_identical_at_the_frame_size(ops):
    """tg_convt3x3s2_z_fwd_form 3 (round 6, what the rule picks at this size): whole rounds of four-row workgroups and a
    second launch of two-row workgroups for the remaining rows -- against the single-launch tiled form (0), bit for bit,
    at the 268x640 -> 536x1280 shape of the inference frame; rows that the first launch does not cover must not be
    touched by it (the buffer is pre-filled)."""
    n, cin, cout, cz, h, w = 1, 64, 64, 3, 268, 640
    x = dev(rs(1, (n, cin, h, w), -1, 1))
    wt = rs(2, (cin, cout, 3, 3), -1, 1) / (1.5 * cin ** 0.5)
    b = dev(rs(3, (cout,), -0.5, 0.5))
    wo = rs(4, (cz, cout, 3, 3), -1, 1) / (3.0 * cout ** 0.5)
    pk, _, _, _ = ops.pack_conv3x3(dev(wt), transposed=True)
    wz = ops.convt_pack_wz(dev(wo))
    ref = ops.convt3x3s2_z(x, pk, b, wz, cz, cout, act=1, form=0)
    for form in (3, -1):
        out = torch.full((n, 32, 2 * h, 2 * w), 7.0, device='cuda')
        ops.convt3x3s2_z(x, pk, b, wz, cz, cout, act=1, form=form, out=out)
        assert torch.equal(out[:, :27], ref[:, :27]), (form, (out[:, :27] - ref[:, :27]).abs().max().item())
        assert bool((out[:, 27:] == 7.0).all()), form


def test_convt_z_rejects_the_removed_forms(ops):
    """Forms 1 and 2 (the streaming form, removed) are invalid arguments now, and the error names the valid ones."""
    from tecogan_pytorch_amd._lib import TecoganHipError
    n, cin, cout, cz, h, w = 1, 64, 64, 3, 12, 20
    x, b = dev(rs(1, (n, cin, h, w), -1, 1)), dev(rs(3, (cout,), -0.5, 0.5))
    pk, _, _, _ = ops.pack_conv3x3(dev(rs(2, (cin, cout, 3, 3), -1, 1)), transposed=True)
    wz = ops.convt_pack_wz(dev(rs(4, (cz, cout, 3, 3), -1, 1)))
    for form in (1, 2):
        with pytest.raises(TecoganHipError) as e:
            ops.convt3x3s2_z(x, pk, b, wz, cz, cout, act=1, form=form)
        msg = str(e.value)
        assert f'form={form}' in msg and all(v in msg for v in ('-1 the rule', '0 tiled', '3 tiled')), msg


@pytest.mark.parametrize('n,cz,h,w,up', [(1, 3, 48, 80, ('BD', 4)), (2, 3, 44, 132, ('BI', 2)), (1, 3, 20, 36, ('BD', 2)),
                                         (1, 1, 17, 72, None), (2, 2, 8, 4, None), (1, 3, 536, 1280, ('BD', 4))])
def test_convout_tail_forms_are_bit_identical_and_match_the_reference(ops, n, cz, h, w, up):
    """tg_convout_tail_form (conv_out's 9-tap shift-add of the Z planes + bias + `+= upsample_func(lr_curr)` +
    float32_to_uint8; tecogan_nets.py:131,145, data_utils.py:80-87): the four-pixels-per-thread form (round 6) equals the
    one-pixel form bit for bit -- fp32 AND uint8, rows of one and of several threads, both up-samplers -- and both
    are the reference composition."""
    import torch.nn.functional as F
    z = rs(1, (n, 32, h, w), -1, 1)
    b = rs(2, (cz,), -0.5, 0.5)
    ref = torch.zeros(n, cz, h, w, dtype=torch.float64)
    zp = F.pad(z.double(), (1, 1, 1, 1))
    for ky in range(3):
        for kx in range(3):
            ref += zp[:, (ky * 3 + kx) * cz:(ky * 3 + kx + 1) * cz, ky:ky + h, kx:kx + w]
    ref += b.double().view(1, cz, 1, 1)
    kw = {}
    if up:
        deg, s_ = up
        src = rs(3, (n, cz, h // s_, w // s_), 0, 1)
        ref += O.upsample(src, s_, deg).double()
        kw = dict(up_src=dev(src), up_mode=ops.UP_BICUBIC if deg == 'BD' else ops.UP_BILINEAR, up_scale=s_)
    y0, u0 = ops.convout_tail(dev(z), cz, dev(b), want_u8=True, form=0, **kw)
    y1, u1 = ops.convout_tail(dev(z), cz, dev(b), want_u8=True, form=1, **kw)
    ya = ops.convout_tail(dev(z), cz, dev(b), **kw)
    assert err(y0, ref) <= 2e-5, err(y0, ref)
    assert torch.equal(y0, y1) and torch.equal(u0, u1) and torch.equal(ya, y0), ((y0 - y1).abs().max().item(), int((u0 != u1).sum()))
    assert torch.equal(u0.cpu(), torch.from_numpy(O.float32_to_uint8(y0.cpu().numpy())).permute(0, 2, 3, 1))


@pytest.mark.parametrize('cin,cout,h,w,act,up', [
    (32, 2, 16, 40, 3, None), (64, 3, 48, 80, 0, ('BD', 4)), (64, 3, 44, 132, 0, ('BI', 2)),
    (64, 3, 20, 36, 0, ('BD', 2)), (9, 4, 7, 5, 1, None), (64, 1, 17, 70, 0, None)])
def test_conv3x3_small(ops, cin, cout, h, w, act, up):
    import torch.nn.functional as F
    x = rs(1, (2, cin, h, w), -1, 1)
    wt = rs(2, (cout, cin, 3, 3), -1, 1) / (3.0 * cin ** 0.5)
    b = rs(3, (cout,), -0.5, 0.5)
    ref = F.conv2d(x.double(), wt.double(), b.double(), padding=1)
    ref = {0: ref, 1: torch.relu(ref), 3: torch.tanh(ref) * 24}[act]
    kw = {}
    if up:
        deg, s = up
        src = rs(6, (2, cout, h // s, w // s))
        ref = ref + O.upsample(src, s, deg).double()
        kw = dict(up_src=dev(src), up_mode=ops.UP_MODE[deg], up_scale=s)
    out = ops.conv3x3_small(dev(x), dev(wt), dev(b), act, **kw)
    tol = 2e-4 if act == 3 else 1e-5
    assert err(out, ref) <= tol, err(out, ref)


@pytest.mark.parametrize('n,cin,cout,h,w,act,with_res', [
    (2, 64, 3, 128, 128, 0, True), (2, 64, 3, 6, 64, 0, True), (3, 40, 2, 9, 12, 1, False), (1, 64, 4, 5, 200, 2, True),
    (2, 3, 3, 10, 8, 0, False), (36, 32, 2, 16, 16, 3, False)])
def test_conv3x3_small_four_row_form(ops, n, cin, cout, h, w, act, with_res):
    """The small-cout kernel's form for launches of few tiles (4-row tiles, the waves of a workgroup split the
    input channels): with an explicit residual tensor (tg_conv3x3_small_fwd_res, the training step's conv_out)
    and without (picked by tg_conv3x3_small_fwd itself)."""
    import torch.nn.functional as F
    x = rs(1, (n, cin, h, w), -1, 1)
    wt = rs(2, (cout, cin, 3, 3), -1, 1) / (3.0 * cin ** 0.5)
    b = rs(3, (cout,), -0.5, 0.5)
    ref = F.conv2d(x.double(), wt.double(), b.double(), padding=1)
    ref = {0: ref, 1: torch.relu(ref), 2: F.leaky_relu(ref, 0.2), 3: torch.tanh(ref) * 24}[act]
    res = rs(4, (n, cout, h, w), -1, 1) if with_res else None
    if with_res:
        ref = ref + res.double()
        assert ops.conv3x3_small_res_ok(dev(x), dev(res))
    out = ops.conv3x3_small(dev(x), dev(wt), dev(b), act, res=dev(res) if with_res else None)
    tol = 2e-4 if act == 3 else 1e-5
    assert err(out, ref) <= tol, err(out, ref)


@pytest.mark.parametrize('deg,s,h,w', [('BD', 4, 22, 40), ('BD', 4, 21, 37), ('BI', 2, 22, 40),
                                       ('BD', 2, 19, 33), ('BI', 4, 16, 24)])
def test_fused_flowup_warp_s2d_vs_oracle(ops, deg, s, h, w):
    """= space_to_depth(backward_warp(hr_prev, s*up(reflect_pad(lr_flow)))) of the oracle."""
    fh, fw = h // 8 * 8, w // 8 * 8
    lr_flow = rs(1, (2, 2, fh, fw), -5, 5)
    hr_prev = rs(2, (2, 3, s * h, s * w))
    pad = O.reflect_pad_br(lr_flow, h - fh, w - fw)
    hr_flow = s * O.upsample(pad, s, deg)
    ref = O.space_to_depth(O.backward_warp(hr_prev, hr_flow), s)
    out, hf = ops.flowup_warp_s2d(dev(lr_flow), dev(hr_prev), h, w, s, ops.UP_MODE[deg],
                                  want_hr_flow=True)
    assert err(hf, hr_flow) <= 2e-5
    # white-noise image: a 1-ulp difference in the sampling position is worth ~|grad| * 4e-6
    assert err(out, ref) <= 5e-5, err(out, ref)


def _camera_flow(n, fh, fw, pan, zoom, roll, seed):
    """LR flow of a camera motion: per-clip pan (LR px) + zoom + roll about the centre."""
    g = np.random.RandomState(seed)
    ys, xs = np.meshgrid(np.arange(fh, dtype=np.float32) - fh / 2,
                         np.arange(fw, dtype=np.float32) - fw / 2, indexing='ij')
    out = np.empty((n, 2, fh, fw), np.float32)
    for i in range(n):
        px, py = (g.rand(2) - 0.5) * 2 * pan
        z, r = (g.rand() - 0.5) * 2 * zoom, (g.rand() - 0.5) * 2 * roll
        out[i, 0] = px + z * xs - r * ys
        out[i, 1] = py + z * ys + r * xs
    return torch.from_numpy(out)


@pytest.mark.parametrize('deg,s,h,w', [('BD', 4, 20, 72), ('BI', 2, 24, 136), ('BD', 2, 18, 130),
                                       ('BI', 4, 12, 66)])
@pytest.mark.parametrize('pan,zoom,roll', [(0.0, 0.0, 0.0), (1.0, 0.01, 0.005), (3.0, 0.05, 0.02),
                                           (40.0, 0.0, 0.0)])
def test_fused_flowup_warp_s2d_smooth_flow(ops, deg, s, h, w, pan, zoom, roll):
    """Smooth flows take the kernel's shared-gather path (two adjacent pixels served by one
    16-byte lane); several 256-pixel segments per row incl. a partial one; a 40-LR-pixel pan
    pushes most samples onto the clamped frame border."""
    fh, fw = h // 2 * 2, w // 2 * 2
    lr_flow = _camera_flow(2, fh, fw, pan, zoom, roll, seed=h + w)
    hr_prev = rs(5, (2, 3, s * h, s * w))
    pad = O.reflect_pad_br(lr_flow, h - fh, w - fw)
    hr_flow = s * O.upsample(pad, s, deg)
    ref = O.space_to_depth(O.backward_warp(hr_prev, hr_flow), s)
    out, hf = ops.flowup_warp_s2d(dev(lr_flow), dev(hr_prev), h, w, s, ops.UP_MODE[deg],
                                  want_hr_flow=True)
    assert err(hf, hr_flow) <= 2e-5 * max(1.0, pan)
    assert err(out, ref) <= 5e-5 * max(1.0, pan / 4), err(out, ref)


def test_fused_flowup_warp_s2d_many_clips_bitwise(ops):
    """> 2048 tiles per launch switches the kernel to 2 rows per thread; same arithmetic, so
    the batched launch must reproduce the per-clip launches bit for bit."""
    s, h, w, n = 4, 48, 64, 44
    lr_flow = torch.cat([_camera_flow(n // 2, h, w, 2.0, 0.02, 0.01, seed=3),
                         rs(8, (n // 2, 2, h, w), -4, 4)])
    hr_prev = rs(9, (n, 3, s * h, s * w))
    fl, pv = dev(lr_flow), dev(hr_prev)
    big = ops.flowup_warp_s2d(fl, pv, h, w, s, ops.UP_BICUBIC)
    for i in (0, 7, n // 2, n - 1):
        one = ops.flowup_warp_s2d(fl[i:i + 1].contiguous(), pv[i:i + 1].contiguous(), h, w, s,
                                  ops.UP_BICUBIC)
        assert torch.equal(big[i:i + 1], one), i
    ref = O.space_to_depth(O.backward_warp(hr_prev[:2], s * O.upsample(lr_flow[:2], s, 'BD')), s)
    assert err(big[:2], ref) <= 5e-5


# ------------------------------------------------------------------- networks
CFGS = [('BD', 4), ('BI', 2), ('BD', 2)]


@pytest.mark.parametrize('deg,s', CFGS)
def test_fnet_vs_reference(golden, deg, s):
    g = golden(f'gen_{deg}{s}')
    net, _ = make_net(deg, s)
    for hw in ('22x40', '16x24'):
        out = net.fnet(dev(g[f'fnet_{hw}_x1']), dev(g[f'fnet_{hw}_x2']))
        assert err(out, g[f'fnet_{hw}_out']) <= 2e-4, hw


@pytest.mark.parametrize('deg,s', CFGS)
def test_srnet_vs_reference(golden, deg, s):
    g = golden(f'gen_{deg}{s}')
    net, _ = make_net(deg, s)
    out = net.srnet(dev(g['srnet_lr']), dev(g['srnet_tran']))
    assert err(out, g['srnet_out']) <= 5e-5


@pytest.mark.parametrize('deg,s', CFGS)
@pytest.mark.parametrize('path', ['plan', 'ops'])
def test_step_vs_reference(golden, deg, s, path):
    g = golden(f'gen_{deg}{s}')
    net, _ = make_net(deg, s)
    for hw in ('22x40', '21x37'):
        args = [dev(g[f'step_{hw}_{k}']) for k in ('lr_curr', 'lr_prev', 'hr_prev')]
        with torch.no_grad():
            out = net.step(*args) if path == 'plan' else net.step_ops(*args)
        ref = g[f'step_{hw}_out']
        assert err(out, ref) <= 1e-4, (hw, err(out, ref))
        dpsnr = O.psnr_float(out.cpu().numpy(), ref)
        assert dpsnr > 80, dpsnr      # i.e. the two outputs differ by < -80 dB


@pytest.mark.parametrize('deg,s', CFGS)
def test_infer_sequence_u8_vs_reference(golden, deg, s):
    g = golden(f'gen_{deg}{s}')
    net, _ = make_net(deg, s)
    out = net.infer_sequence(T(g['infer_lr']), 'cuda')
    ref = g['infer_out_u8']
    assert out.shape == ref.shape and out.dtype == np.uint8
    diff = np.abs(out.astype(np.int16) - ref.astype(np.int16))
    assert diff.max() <= 1 and (diff != 0).mean() < 1e-3, ((diff != 0).mean(), diff.max())
    # BASELINE metric: PSNR of build vs reference output (Y channel) -- identical up to ties
    for t in range(out.shape[0]):
        p = O.psnr(ref[t], out[t])
        assert p == np.inf or p > 60


def test_step_batched_clips_equal_independent_steps():
    """n > 1 through the plan (several clips per GPU in one launch list) == per-clip steps."""
    net, _ = make_net('BD', 4)
    lc, lp = dev(rs(1, (3, 3, 24, 40), 0, 1)), dev(rs(2, (3, 3, 24, 40), 0, 1))
    hp = dev(rs(3, (3, 3, 96, 160), 0, 1))
    with torch.no_grad():
        both = net.step(lc, lp, hp)
        for i in range(3):
            one = net.step(lc[i:i + 1], lp[i:i + 1], hp[i:i + 1])
            assert err(both[i:i + 1], one) <= 2e-6      # tile shapes may differ (split-K choice)


@pytest.mark.parametrize('deg,s,h,w', [('BD', 4, 8, 8), ('BI', 2, 9, 15), ('BD', 2, 15, 8)])
def test_step_minimum_sizes_vs_oracle(deg, s, h, w):
    """Smallest legal frames (FNet bottleneck 1x1, reflect pad up to 7 rows/cols)."""
    net, sd = make_net(deg, s)
    lc, lp, hp = rs(1, (1, 3, h, w), 0, 1), rs(2, (1, 3, h, w), 0, 1), rs(3, (1, 3, s * h, s * w), 0, 1)
    with torch.no_grad():
        ref = O.frnet_step(sd, lc, lp, hp, s, deg)
        out = net.step(dev(lc), dev(lp), dev(hp))
    assert err(out, ref) <= 1e-4


def test_invalid_shapes_raise():
    from tecogan_pytorch_amd._lib import TecoganHipError
    net, _ = make_net('BD', 4)
    with pytest.raises(TecoganHipError):          # below the 8x8 minimum of the flow estimator
        net.step(dev(rs(1, (1, 3, 6, 12))), dev(rs(2, (1, 3, 6, 12))), dev(rs(3, (1, 3, 24, 48))))
    with pytest.raises(TecoganHipError):          # hr_prev of the wrong size
        net.step(dev(rs(1, (1, 3, 16, 16))), dev(rs(2, (1, 3, 16, 16))), dev(rs(3, (1, 3, 32, 32))))
    out = net.infer_sequence(torch.rand(1, 3, 16, 24), 'cuda')        # single-frame clip
    assert out.shape == (1, 64, 96, 3)


def test_pipelined_clip_inference_is_deterministic_and_matches_single_stream():
    """The two-stream pipeline (batched FNet on the side stream, SRNet on the main one) must be
    race-free: repeated runs are bit-identical.  Against the frame-by-frame path only the
    split-K factor of some batched FNet layers differs (summation order): one uint8 level on a
    handful of pixels at most."""
    net, _ = make_net('BD', 4)
    clip = smooth_clip(9, 3, 40, 64, seed=4)
    a = net.infer_sequence(clip, 'cuda', pipeline=False)
    first = None
    for _ in range(4):
        b = net.infer_sequence(clip, 'cuda', pipeline=True)
        if first is None:
            first = b
        assert np.array_equal(first, b)
    d = np.abs(a.astype(np.int16) - first.astype(np.int16))
    assert d.max() <= 1 and (d > 0).mean() <= 2e-3, (d.max(), (d > 0).mean())
    # the same launch list on ONE stream (pipeline='one_stream'): identical kernels, identical bits --
    # from a host clip (streamed uploads / downloads on the copy stream) and from a device clip
    assert np.array_equal(net.infer_sequence(clip, 'cuda', pipeline='one_stream'), first)
    one = net.infer_sequence(clip.cuda(), 'cuda', pipeline='one_stream', return_device_tensor=True)
    assert np.array_equal(one.cpu().numpy(), first)


def test_pipelined_clip_reusing_both_flow_slots_matches_every_other_path(monkeypatch):
    """With the default batch size no short clip writes a flow slot a second time while the other stream is live.
    TG_FNET_BATCH=2 cuts 9 frames into 3, 2, 2, 2: slots 0 and 1 are both written twice.  (That the wait for the batch
    two back is enqueued is asserted by tests/test_infer_schedule_cpu.py; a race at this size would rarely show here.)
    The pipelined clip is bit-identical run after run, to the same launches on ONE stream (no concurrency)
    and to infer_stream fed frame by frame (the same enqueue_batch on ring slots); against the frame-by-frame path the
    neighbouring tests' bound holds (summation order of the batched FNet layers)."""
    monkeypatch.setenv('TG_FNET_BATCH', '2')
    from tecogan_pytorch_amd.models.networks import frnet_infer
    assert frnet_infer.clip_batches(9, *frnet_infer.stream_batch_sizes()) == [(0, 3), (3, 2), (5, 2), (7, 2)]
    net, _ = make_net('BD', 4)
    clip = smooth_clip(9, 3, 24, 40, seed=31)
    first = net.infer_sequence(clip, 'cuda', pipeline=True)
    for _ in range(2):
        assert np.array_equal(net.infer_sequence(clip, 'cuda', pipeline=True), first)
    assert np.array_equal(net.infer_sequence(clip, 'cuda', pipeline='one_stream'), first)
    streamed = np.concatenate([chunk.copy() for chunk in net.infer_stream((f for f in clip), 'cuda')], 0)
    assert np.array_equal(streamed, first)
    d = np.abs(net.infer_sequence(clip, 'cuda', pipeline=False).astype(np.int16) - first.astype(np.int16))
    print('pipeline=True (TG_FNET_BATCH=2) against pipeline=False: max %d, differing %.3g' % (d.max(), (d > 0).mean()))
    assert d.max() <= 1 and (d > 0).mean() <= 2e-3, (d.max(), (d > 0).mean())


# --------------------------------------------------- BASELINE full-size checks
def test_fullsize_A_digest_vs_reference(golden):
    """config 1/2 shape: 4xBD, LR 1x3x134x320, seeded uniform inputs."""
    g = golden('fullsize')
    net, _ = make_net('BD', 4)
    h, w, s = 134, 320, 4
    with torch.no_grad():
        out = net.step(dev(rs(100, (1, 3, h, w))), dev(rs(101, (1, 3, h, w))),
                       dev(rs(102, (1, 3, s * h, s * w))))
    flat = out.double().cpu().reshape(-1)
    idx = T(g['full_A_sample_idx'])
    assert (flat[idx].float().numpy() - g['full_A_samples']).__abs__().max() <= 3e-4
    assert abs(flat.mean().item() - float(g['full_A_mean'])) <= 1e-5
    assert abs(flat.norm().item() - float(g['full_A_l2'])) <= 1e-4 * flat.numel() ** 0.5


@pytest.mark.parametrize('deg,s,h,w', [('BD', 4, 134, 320), ('BI', 2, 268, 640)])
def test_fullsize_step_vs_oracle_and_psnr(deg, s, h, w):
    """Full BASELINE sizes against the oracle on a smooth (flow-like) clip:
    frame 0 from zero state, frame 1 recurrent; fp32 tolerance 2e-4 abs and the
    north-star bound |PSNR(build) - PSNR(reference)| <= 1e-3 dB against a
    common pseudo ground truth."""
    net, sd = make_net(deg, s)
    clip = smooth_clip(2, 3, h, w, seed=11)
    with torch.no_grad():
        z_lr, z_hr = torch.zeros(1, 3, h, w), torch.zeros(1, 3, s * h, s * w)
        o0 = O.frnet_step(sd, clip[0:1], z_lr, z_hr, s, deg)
        o1 = O.frnet_step(sd, clip[1:2], clip[0:1], o0, s, deg)
        g0 = net.step(dev(clip[0:1]), dev(z_lr), dev(z_hr))
        g1 = net.step(dev(clip[1:2]), dev(clip[0:1]), g0)
    assert err(g0, o0) <= 2e-4 and err(g1, o1) <= 2e-4, (err(g0, o0), err(g1, o1))
    gt = O.upsample(clip[1:2], s, deg).numpy()
    d = abs(O.psnr_float(g1.cpu().numpy(), gt) - O.psnr_float(o1.numpy(), gt))
    assert d <= 1e-3, d


def test_fullsize_properties(ops):
    """Size-independent properties at HR 536x1280."""
    H, W = 536, 1280
    x = dev(rs(7, (1, 3, H, W)))
    # zero flow is the identity and integer flow a pure shift, up to the fp32
    # resolution of the normalised-coordinate round trip (ulp(1279) ~ 1.2e-4 px,
    # times a white-noise gradient of <= 1 per px)
    assert err(ops.backward_warp(x, torch.zeros(1, 2, H, W, device='cuda')), x) <= 5e-4
    fl = torch.zeros(1, 2, H, W, device='cuda'); fl[:, 0] = 3.0; fl[:, 1] = -2.0
    y = ops.backward_warp(x, fl)
    assert err(y[..., 2:H, 0:W - 3], x[..., 0:H - 2, 3:W]) <= 5e-4
    # space_to_depth is a permutation: sorted values identical, and depth->space inverts it
    s2d = ops.space_to_depth(x, 4)
    back = s2d.view(1, 4, 4, 3, H // 4, W // 4).permute(0, 3, 4, 1, 5, 2).reshape(1, 3, H, W)
    assert torch.equal(back, x)
    # conv linearity: conv(a x1 + b x2) = a conv(x1) + b conv(x2) (bias-free)
    wt = dev(rs(8, (64, 64, 3, 3), -1, 1) / 24.0)
    pk, _, _, ocb = ops.pack_conv3x3(wt)
    x1, x2 = dev(rs(9, (1, 64, 134, 320), -1, 1)), dev(rs(10, (1, 64, 134, 320), -1, 1))
    lhs = ops.conv3x3(2.0 * x1 - 0.5 * x2, pk, None, 64, 64, ocb)
    rhs = 2.0 * ops.conv3x3(x1, pk, None, 64, 64, ocb) - 0.5 * ops.conv3x3(x2, pk, None, 64, 64, ocb)
    assert err(lhs, rhs) <= 2e-5
    # determinism: same launch twice is bit-identical
    assert torch.equal(ops.conv3x3(x1, pk, None, 64, 64, ocb), ops.conv3x3(x1, pk, None, 64, 64, ocb))


def test_step_is_deterministic_and_stateless():
    net, _ = make_net('BD', 4)
    a = [dev(rs(100 + i, sh)) for i, sh in enumerate([(1, 3, 134, 320), (1, 3, 134, 320),
                                                      (1, 3, 536, 1280)])]
    with torch.no_grad():
        o1 = net.step(*a).clone()
        net.step(a[1], a[0], a[2])          # disturb the workspace
        o2 = net.step(*a)
    assert torch.equal(o1, o2)


def test_missing_library_is_loud(monkeypatch):
    from tecogan_pytorch_amd import _lib
    monkeypatch.setattr(_lib, '_lib', None)
    monkeypatch.setattr(_lib, 'LIB_PATH', '/nonexistent/libtecogan_hip.so')
    with pytest.raises(_lib.TecoganHipError):
        _lib.lib()


@pytest.mark.parametrize('frames', [1, 2, 3, 9, 17])
def test_infer_sequence_batched_flow_pipeline_matches_frame_by_frame(frames):
    """pipeline=True estimates the flows of up to 8 frame pairs per batched FNet pass (full
    batches plus a tail batch) and feeds them to the per-frame SRNet plan; pipeline=False runs
    FRNet.step frame by frame.  Same arithmetic up to the split-K choices of the batched FNet
    layers (summation order), so the uint8 frames agree to one level on at most a few pixels."""
    net, _ = make_net('BD', 4)
    clip = smooth_clip(frames, 3, 24, 40, seed=31)
    a = net.infer_sequence(clip, 'cuda', pipeline=True)
    b = net.infer_sequence(clip, 'cuda', pipeline=False)
    assert a.shape == b.shape == (frames, 96, 160, 3) and a.dtype == np.uint8
    d = np.abs(a.astype(np.int16) - b.astype(np.int16))
    assert d.max() <= 1, d.max()
    assert (d > 0).mean() <= 2e-3, (d > 0).mean()


@pytest.mark.parametrize('pipeline', [True, False])
def test_infer_sequence_batch_of_clips_matches_clip_by_clip(pipeline):
    """(k, t, c, h, w) input: k independent clips advanced in lockstep through one launch list
    (batched uint8 output of the fused HR tail).  Against each clip alone: same arithmetic up to
    the split-K / tile choices of differently sized launches."""
    net, _ = make_net('BD', 4)
    clips = torch.stack([smooth_clip(11, 3, 24, 40, seed=50 + i) for i in range(3)])
    both = net.infer_sequence(clips, 'cuda', pipeline=pipeline)
    assert both.shape == (3, 11, 96, 160, 3) and both.dtype == np.uint8
    dev_out = net.infer_sequence(clips.cuda(), 'cuda', pipeline=pipeline, return_device_tensor=True)
    assert np.array_equal(dev_out.cpu().numpy(), both)
    for i in range(3):
        one = net.infer_sequence(clips[i], 'cuda', pipeline=pipeline)
        d = np.abs(both[i].astype(np.int16) - one.astype(np.int16))
        assert d.max() <= 1 and (d > 0).mean() <= 2e-3, (i, d.max(), (d > 0).mean())
