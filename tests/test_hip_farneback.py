"""GPU: tg_farneback.hip against its specification tests/farneback_ref.py.

Per stage, on the kernel's own input: gray exact; the linear stages (level image, polynomial expansion, box mean)
inside a derived fp32 bound: each pass of K taps contributes at most (K + 2) 2^-24 S -- K - 1 additions, one product,
the tap's own rounding and one more for a paired tap's inner sum -- with S the same sums over absolute values, and the
passes of a stage add up; the non-linear stages (update matrices, solve, flow resize) triangulated on identical
inputs.  Whole flows are triangulated: relL2(HIP, spec64) <= 2 x relL2(alt32, spec64), both right-hand quantities from
the CPU, and max |HIP - spec64| <= 1e-3 px.  Then determinism, layout, the end-point-error mean and both evaluators.

Shapes: 40x56 (one level, the border zone is a large share), 72x100 (two levels, exact halves), 75x101 (odd sizes,
half-even rounding), 256x264 (four levels, coarsest 32x33)."""
import functools

import numpy as np
import pytest
import torch

import tecogan_pytorch_amd  # noqa: F401
from tecogan_pytorch_amd import _lib as L
from tecogan_pytorch_amd import ops
from tests import farneback_ref as F
from tests.farneback_fixture import sequence_pair, shifted_texture

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
SHAPES = ((40, 56), (72, 100), (75, 101), (256, 264))


# ---- fixtures: contents x shapes, references computed once ---------------------------------------------------
@functools.lru_cache(maxsize=None)
def frames(kind, h, w):
    """(prev, next) uint8 gray frames."""
    if kind == 'flats':       # a texture with saturated flats (about 20 % of the pixels at 0 or 255), moved by (2.25, -1.5)
        a, b = shifted_texture(h, w, (2.25, -1.5), seed=11, gain=816.0, offset=-280.5)
        sat = ((a == 0) | (a == 255)).mean()
        assert 0.1 < sat < 0.35, sat
        return a, b
    if kind == 'noise':       # uniform noise rolled by one pixel
        a = np.random.default_rng(5).integers(0, 256, (h, w)).astype(np.uint8)
        return a, np.roll(a, 1, 1)
    if kind == 'six':         # a 6-pixel shift: samples leave the frame, the "outside" branch of step 6 runs
        return shifted_texture(h, w, (6.0, 0.0), seed=12)
    if kind == 'const':
        return np.full((h, w), 200, np.uint8), np.full((h, w), 200, np.uint8)
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def reference(kind, h, w):
    a, b = frames(kind, h, w)
    return F.farneback(a, b), F.alt32(a, b)


CASES = [('flats', h, w) for h, w in SHAPES] + [('noise', h, w) for h, w in SHAPES] + \
        [('six', 40, 56), ('const', 40, 56), ('const', 75, 101)]


def gray_rgb(g):
    return np.repeat(g[..., None], 3, -1)       # R = G = B = g: the gray kernel returns g (16384 g + 8192) >> 14


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def hip_flow(prev, nxt):
    return ops.farneback_flow(dev(np.stack([gray_rgb(prev), gray_rgb(nxt)])))[0].cpu().numpy()


def rel_l2(a, b):
    return float(np.linalg.norm(a.astype(np.float64) - b) / np.linalg.norm(b))


# ---- stage launches through the C ABI ------------------------------------------------------------------------
def _call(name, *args):
    L.check(getattr(L.lib(), name)(*args), name)
    torch.cuda.synchronize()


def st_gray(rgb, h, w):
    t, fh, fw, _ = rgb.shape
    out = torch.empty(t, h, w, dtype=torch.uint8, device='cuda')
    _call('tg_fb_gray_u8', rgb.data_ptr(), t, fh, fw, h, w, out.data_ptr(), None)
    return out


def st_level(gray, k):
    n, h, w = gray.shape
    lh, lw = F.level_size(h, w, k)
    tmp = torch.empty(n, h, w, device='cuda')
    out = torch.empty(n, lh, lw, device='cuda')
    _call('tg_fb_level_image', gray.data_ptr(), n, h, w, k, tmp.data_ptr(), out.data_ptr(), None)
    return out


def st_polyexp(img):
    n, h, w = img.shape
    out = torch.empty(n, 5, h, w, device='cuda')
    _call('tg_fb_polyexp', img.data_ptr(), n, h, w, out.data_ptr(), None)
    return out


def st_update(R, flow):
    p, h, w, _ = flow.shape
    assert R.shape[0] == p + 1
    out = torch.empty(p, 5, h, w, device='cuda')
    _call('tg_fb_update_matrices', R.data_ptr(), flow.data_ptr(), out.data_ptr(), p, h, w, None)
    return out


def st_blur_solve(M, want_box=True):
    p, _, h, w = M.shape
    flow = torch.empty(p, h, w, 2, device='cuda')
    box = torch.empty(p, 5, h, w, device='cuda') if want_box else None
    _call('tg_fb_blur_solve', M.data_ptr(), flow.data_ptr(), box.data_ptr() if want_box else None, p, h, w, None)
    return flow, box


def st_resize(flow, oh, ow):
    p, h, w, _ = flow.shape
    out = torch.empty(p, oh, ow, 2, device='cuda')
    _call('tg_fb_resize_flow', flow.data_ptr(), h, w, out.data_ptr(), oh, ow, p, None)
    return out


# ---- bounds of the linear stages -----------------------------------------------------------------------------
def _abs_pass(a, taps, axis):
    r = len(taps) // 2
    pad = np.pad(a, [(r, r) if ax == axis else (0, 0) for ax in (0, 1)], mode='edge')
    n = a.shape[axis]
    return sum(abs(t) * (pad[i:i + n] if axis == 0 else pad[:, i:i + n]) for i, t in enumerate(taps))


def polyexp_abs_sums(img):
    """S of the five outputs: the expansion with |taps| on |img| and |ig..| in the combinations."""
    g, xg, xxg, (ig11, ig03, ig33, ig55) = F.poly_constants()
    a = np.abs(img.astype(np.float64))
    v0, v1, v2 = (_abs_pass(a, t, 0) for t in (g, xg, xxg))
    b1, b2, b4 = (_abs_pass(v0, t, 1) for t in (g, xg, xxg))
    b3, b5, b6 = _abs_pass(v1, g, 1), _abs_pass(v1, xg, 1), _abs_pass(v2, g, 1)
    return np.stack([b3 * abs(ig11), b2 * abs(ig11), b1 * abs(ig03) + b6 * abs(ig33),
                     b1 * abs(ig03) + b4 * abs(ig33), b5 * abs(ig55)])


# ---- stages --------------------------------------------------------------------------------------------------
def test_gray_exact_and_windowed():
    rng = np.random.default_rng(0)
    rgb = rng.integers(0, 256, (3, 45, 77, 3)).astype(np.uint8)
    rgb[0, 0, :6] = [[255, 255, 255], [0, 0, 0], [255, 0, 0], [0, 255, 0], [0, 0, 255], [1, 1, 1]]
    got = st_gray(dev(rgb), 40, 56).cpu().numpy()
    assert (got == F.gray_u8(rgb[:, :40, :56])).all()
    assert (st_gray(dev(rgb), 45, 77).cpu().numpy() == F.gray_u8(rgb)).all()


@pytest.mark.parametrize('kind,h,w', [('flats', 72, 100), ('noise', 75, 101), ('noise', 256, 264), ('flats', 40, 56)])
def test_level_image_and_polyexp_bounds(kind, h, w):
    a, b = frames(kind, h, w)
    gray = dev(np.stack([a, b]))
    for k in range(F.top_level(h, w) + 1):
        img = st_level(gray, k).cpu().numpy()
        ks = len(F.blur_taps(k))
        worst = 0.0
        for i, g in enumerate((a, b)):
            E = F.level_image(g, k)                                   # all weights and values >= 0: S = E
            bound = (2 * (ks + 2) + 2 * (2 + 2)) * U * E              # two blur passes of ks taps, two lerps of 2
            err = np.abs(img[i] - E)
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()) if E.any() else 0.0)
            assert (err <= bound).all(), (k, i, float(err.max()))
        print(f'level image {kind} {h}x{w} k={k}: worst error / bound {worst:.3f}')
        if k == 0:
            assert (img[0] == F.level_image(a, 0)).all()               # [1/4 1/2 1/4] of integers is exact in fp32
        R = st_polyexp(dev(img)).cpu().numpy()
        for i in range(2):
            E = F.polyexp(img[i].astype(np.float64))
            S = polyexp_abs_sums(img[i])
            bound = (2 * (11 + 2) + (2 + 2)) * U * S                  # two passes of 11 taps + the 2-term combination
            err = np.abs(R[i] - E)
            assert (err <= bound).all(), (k, i, float((err / np.maximum(bound, 1e-300)).max()))
        print(f'polyexp {kind} {h}x{w} k={k}: worst error / bound '
              f'{float((err / np.maximum(bound, 1e-300)).max()):.3f}')


def test_polyexp_of_a_constant_region_has_exact_zeros():
    img = torch.full((1, 40, 56), 200.0, device='cuda')
    R = st_polyexp(img).cpu().numpy()[0]
    assert not R[[0, 1, 4]].any()


@pytest.mark.parametrize('kind,h,w', [('flats', 40, 56), ('flats', 75, 101), ('six', 40, 56), ('noise', 72, 100)])
def test_update_box_solve_resize_on_identical_inputs(kind, h, w):
    """Level 0 of one pair, every stage fed with what the kernels produced before it."""
    a, b = frames(kind, h, w)
    img = st_level(dev(np.stack([a, b])), 0)
    R = st_polyexp(img)
    flow0 = dev((np.array([6.0, 0.0] if kind == 'six' else [2.25, -1.5], np.float32) +
                 np.random.default_rng(1).normal(0, 0.3, (1, h, w, 2)).astype(np.float32)))
    M = st_update(R, flow0)
    Rn, fn = R.cpu().numpy(), flow0.cpu().numpy()[0]
    if kind == 'six':                                                  # the outside branch is taken
        fx = np.arange(w, dtype=np.float32)[None, :] + fn[..., 0]
        assert (fx >= w - 1).mean() > 0.05
    # update matrices: triangulated on identical inputs
    E = F.update_matrices(Rn[0], Rn[1], fn)
    A = F.update_matrices(Rn[0], Rn[1], fn, np.float32)
    d_hip, d_alt = rel_l2(M.cpu().numpy()[0], E), rel_l2(A, E)
    print(f'update {kind} {h}x{w}: relL2 HIP {d_hip:.3e} alt32 {d_alt:.3e}')
    assert d_hip <= 2 * d_alt
    # box mean: derived bound
    flow1, box = st_blur_solve(M)
    Mn = M.cpu().numpy()[0]
    E = F.box_mean(Mn.astype(np.float64))
    S = F.box_mean(np.abs(Mn).astype(np.float64))
    bound = 2 * (15 + 2) * U * S
    err = np.abs(box.cpu().numpy()[0] - E)
    print(f'box {kind} {h}x{w}: worst error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}')
    assert (err <= bound).all()
    assert torch.equal(st_blur_solve(M, want_box=False)[0], flow1)
    # solve: on the kernel's own box means
    Bn = box.cpu().numpy()[0]
    E, A = F.solve(Bn.astype(np.float64)), F.solve(Bn, np.float32)
    d_hip, d_alt = rel_l2(flow1.cpu().numpy()[0], E), rel_l2(A, E)
    print(f'solve {kind} {h}x{w}: relL2 HIP {d_hip:.3e} alt32 {d_alt:.3e}')
    assert d_hip <= 2 * d_alt
    # flow resize to the next finer size of a pyramid whose level 1 this would be
    oh, ow = 2 * h + 1, 2 * w - 1
    up = st_resize(flow1, oh, ow).cpu().numpy()[0]
    f1 = flow1.cpu().numpy()[0]
    E, A = F.resize_flow(f1.astype(np.float64), oh, ow), F.resize_flow(f1, oh, ow, np.float32)
    d_hip, d_alt = rel_l2(up, E), rel_l2(A, E)
    print(f'resize {kind} {h}x{w}: relL2 HIP {d_hip:.3e} alt32 {d_alt:.3e}')
    assert d_hip <= 2 * d_alt


# ---- the whole flow ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind,h,w', CASES)
def test_whole_flow_triangulated(kind, h, w):
    a, b = frames(kind, h, w)
    spec, alt = reference(kind, h, w)
    got = hip_flow(a, b)
    assert got.shape == (h, w, 2) and got.dtype == np.float32
    if kind == 'const':
        assert not got.any() and not spec.any()
        return
    d_hip, d_alt = rel_l2(got, spec), rel_l2(alt, spec)
    worst = float(np.abs(got - spec).max())
    print(f'flow {kind} {h}x{w}: relL2(HIP, spec64) {d_hip:.3e}, relL2(alt32, spec64) {d_alt:.3e}, '
          f'ratio {d_hip / d_alt:.3f}, max |HIP - spec64| {worst:.3e} px')
    assert worst <= 1e-3
    assert d_hip <= 2 * d_alt


def test_identical_frames_give_exactly_zero_flow():
    a, _ = frames('flats', 72, 100)
    assert not hip_flow(a, a).any()


# ---- determinism and layout ----------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def five_frames():
    true, _ = sequence_pair(75, 101, 5, seed=21)
    return true


def test_batch_split_windowed_and_repeat_are_bit_identical(five_frames):
    seq = dev(five_frames)
    whole = ops.farneback_flow(seq)                                    # 4 pairs in one call
    assert whole.shape == (4, 75, 101, 2)
    for i in range(4):
        assert torch.equal(ops.farneback_flow(seq[i:i + 2].contiguous())[0], whole[i]), i
    assert torch.equal(ops.farneback_flow(seq[:3].contiguous()), whole[:2])
    assert torch.equal(ops.farneback_flow(seq), whole)                 # two runs
    big = torch.randint(0, 256, (5, 90, 120, 3), dtype=torch.uint8, device='cuda')
    big[:, :75, :101] = seq                                            # frame_h, frame_w larger than h, w
    assert torch.equal(ops.farneback_flow(big, (75, 101)), whole)
    spec = F.flows_of_sequence(five_frames[:2])
    assert np.abs(whole[0].cpu().numpy() - spec[0]).max() <= 1e-3      # RGB frames whose channels differ


def test_flow_epe_mean(five_frames):
    rng = np.random.default_rng(3)
    fa = rng.normal(0, 2, (3, 72, 100, 2)).astype(np.float32)
    fb = rng.normal(0, 2, (3, 72, 100, 2)).astype(np.float32)
    fb[1] = fa[1]
    win = F.crop_8x8_window(72, 100)
    for window in (win, None, (3, 5, 17, 33)):
        got = ops.flow_epe_mean(dev(fa), dev(fb), window).cpu().numpy()
        exp = F.epe_mean(fa, fb, window)
        n = (window[2] * window[3]) if window else 72 * 100
        # the per-pixel fp32 values are the same numbers; the two fp64 sums differ by their order only:
        # |difference| <= 2 (n - 1) 2^-53 sum|e| / n <= 2 n 2^-53 mean
        assert (np.abs(got - exp) <= 2 * n * 2.0 ** -53 * exp).all(), (window, got, exp)
        assert got[1] == 0.0
    one = ops.flow_epe_mean(dev(fa[2:]), dev(fb[2:]), win).cpu().numpy()
    assert one[0] == ops.flow_epe_mean(dev(fa), dev(fb), win).cpu().numpy()[2]      # any batch split


def test_tof_chunking_does_not_change_values(five_frames, monkeypatch):
    true, pred = sequence_pair(72, 100, 5, seed=22, pred_size=(74, 100))
    t, p = dev(true), dev(pred)
    whole = ops.tof(t, p, F.crop_8x8_window(72, 100))
    monkeypatch.setattr(ops, 'TOF_CHUNK_BYTES', 1)                     # one pair per call, one frame of overlap
    assert torch.equal(ops.tof(t, p, F.crop_8x8_window(72, 100)), whole)
    assert whole.shape == (4,) and whole.dtype == torch.float64


# ---- end to end ----------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def seven():
    true, pred = sequence_pair(72, 100, 7, seed=23, pred_size=(72, 104))
    return true, pred, F.tof(true[2:5], pred[2:5]), F.tof(true, pred, official=False)


def _tof_bound():
    """|tOF_HIP - tOF_spec| <= mean |e_HIP - e_spec| <= 2 x 1.42e-3: each flow is within 1e-3 px per component of
    the specification, so the difference of two flows moves by at most 2e-3 per component."""
    return 2 * np.sqrt(2) * 1e-3


def test_official_metrics_with_tof(seven, golden):
    from tecogan_pytorch_amd.metrics.official import OfficialMetrics
    true, pred, spec, _ = seven
    for lp in (None, _procedural_lpips(golden)):
        plain = OfficialMetrics(lp, device='cuda').compute_sequence(true, pred)
        r = OfficialMetrics(lp, device='cuda', tof=True).compute_sequence(true, pred)
        keys = ('PSNR', 'SSIM', 'LPIPS', 'tOF', 'tLP100') if lp is not None else ('PSNR', 'SSIM', 'tOF')
        assert tuple(list(r)[:len(keys)]) == keys
        assert len(r['tOF']) == 7 - 2 * 2 - 1
        print('tOF official', r['tOF'], 'spec', spec.tolist())
        assert np.abs(np.array(r['tOF']) - spec).max() <= _tof_bound()
        assert 'tOF' not in plain
        for k in plain:                                                # the other columns are bit-identical
            assert plain[k] == r[k], k


def _procedural_lpips(golden):
    """LPIPS with ScalingLayer and the procedural weights, as tests/test_hip_official.py builds it."""
    from lpips_fixture import alexnet_state_dict
    from tecogan_pytorch_amd.metrics.lpips import LPIPS
    g = golden('lpips')
    m = LPIPS(device='cuda', scaling=True)
    m.load_alexnet_state_dict(alexnet_state_dict())
    m.load_lin_state_dict({f'lin{k}.model.1.weight': torch.from_numpy(g[f'lin{k}']) for k in range(5)})
    return m


def test_metric_calculator_with_tof(seven):
    from tecogan_pytorch_amd.metrics.metric_calculator import MetricCalculator
    true, pred, _, spec = seven
    plain = MetricCalculator({'device': 'cuda', 'metric': {'PSNR': {'colorspace': 'y'}}})
    mc = MetricCalculator({'device': 'cuda', 'metric': {'PSNR': {'colorspace': 'y'}, 'tOF': {'backend': 'hip'}}})
    plain.compute_sequence_metrics('s', true, pred)
    mc.compute_sequence_metrics('s', true, pred)
    got = mc.metric_dict['s']
    assert list(got) == ['PSNR', 'tOF'] and len(got['tOF']) == 6 and got['PSNR'] == plain.metric_dict['s']['PSNR']
    print('tOF in-loop', got['tOF'], 'spec', spec.tolist())
    assert np.abs(np.array(got['tOF']) - spec).max() <= _tof_bound()
    mc.gather(['s'])
    assert mc.average()['tOF'] == pytest.approx(np.mean(got['tOF']), rel=1e-12)
