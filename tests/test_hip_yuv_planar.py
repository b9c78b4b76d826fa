"""Planar YUV 4:2:0 / 4:2:2 / 4:4:4 at 8, 10 and 12 bits with BT.601, BT.709 and BT.2020 on the GPU (DESIGN.md section
7l): the three entry points through the C ABI against tests/yuv_planar_ref.py -- both output directions byte for byte and
word for word, the input direction within a derived bound of fp64 -- at shapes that take the wide and the element-wide
form of every layout, with guard bytes around every output; the 4:2:0 instantiations against the four existing entry
points bit for bit; and FRNet.infer_stream(yuv=Yuv(...)) / the CLI against the ops.

Tolerance of the input direction.  The float step is the one of tests/test_hip_yuv.py and tests/test_hip_yuv_depth.py:
yf = ky (Y - yo), then one fma per chroma term on exact integers, coefficients rounded once from fp64, every rounding
at most 2^-24 = 5.96e-8 relative.  The derivation of test_hip_yuv_depth.py is repeated per matrix, for 12-bit limited
range, the largest operands (|yf| <= 3839/3504 = 1.0956, |C - mid| / cs <= 2048/3584 = 0.5714; 8 and 10 bits and full
range are smaller term by term): yf carries 1.306e-7.
  B = fma(bu, du, yf): the rounding of bu on |bu du| <= 0.5714 gb, and the fma's own on a result <= 1.0956 + 0.5714 gb.
    gb = 1.772 (601): 6.03e-8 + 1.256e-7; 1.8556 (709): 6.32e-8 + 1.285e-7; 1.8814 (2020): 6.41e-8 + 1.294e-7.
    With yf: 3.17e-7, 3.22e-7, 3.25e-7.  R has the smaller gain (1.402, 1.5748, 1.4746) and is smaller term by term.
  G = fma(gv, dv, fma(gu, du, yf)) with (gu, gv) = (0.34414, 0.71414), (0.18732, 0.46812), (0.16455, 0.57135):
    1.306e-7 + 5.96e-8 (0.5714 gu + (1.0956 + 0.5714 gu) + 0.5714 gv + (1.0956 + 0.5714 (gu + gv))):
    3.45e-7 (601), 3.12e-7 (709), 3.17e-7 (2020).
The clamp adds nothing.  The bound per matrix is the larger of its two sums: 3.45e-7 (BT.601, G), 3.22e-7 (BT.709, B),
3.25e-7 (BT.2020, B; its B gain is the largest of the three), written as 3.5e-7, 3.3e-7 and 3.3e-7.  The worst observed
value is printed per case."""
import io

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from procedural_weights import generator_state_dict, smooth_clip
from tests import yuv_planar_ref as P
from tests import yuv_ref as R8
from tests.test_hip_yuv_depth import QUIET, _Recorder, _rgb_f32_input, chunkings, float_frames, make_net

DEV = torch.device('cuda', 0)
GUARD = 0xA5
TOL = {'bt601': 3.5e-7, 'bt709': 3.3e-7, 'bt2020': 3.3e-7}        # see the module docstring
E_ARG = -2
ALL_CFGS = [(m, fr, s) for s in P.SITINGS for (m, fr) in P.CONFIGS]          # 2 sitings x 3 matrices x 2 ranges
ONE_CFG = {'420': ('bt2020', False, 'left'), '422': ('bt2020', True, 'left'), '444': ('bt2020', False, 'center')}
OUT_SHAPES = {'444': [(2, 2), (3, 5), (4, 8), (18, 22)], '422': [(2, 2), (3, 6), (5, 10), (4, 8), (64, 130)],
              '420': [(2, 2), (4, 6), (6, 8)]}
OUT_CASES = [(c, H, W) for c in P.CHROMAS for (H, W) in OUT_SHAPES[c]]


def _codes(chroma, matrix, full, siting):
    from tecogan_pytorch_amd import _lib as L
    return L.YUV_CHROMA[chroma], L.YUV_PLANAR_MATRIX[matrix], int(full), L.YUV_SITING[siting]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _guarded(nbytes, pad, dtype):
    """A device buffer of `nbytes` payload bytes with `pad` guard bytes on either side, all set to GUARD; the payload
    starts `pad` bytes into a 256-byte aligned allocation."""
    buf = torch.full((pad + nbytes + pad,), GUARD, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 256 == 0
    return buf, buf[pad:pad + nbytes].view(dtype)


def _guards_intact(buf, pad):
    return bool((buf[:pad] == GUARD).all()) and bool((buf[-pad:] == GUARD).all())


def _placed(arr, in_pad):
    """The bytes of a numpy array on the device, in_pad bytes into a 256-byte aligned allocation -> (holder, address)."""
    raw = torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1))
    hold = torch.empty(in_pad + raw.numel(), dtype=torch.uint8, device=DEV)
    assert hold.data_ptr() % 256 == 0
    hold[in_pad:].copy_(raw)
    return hold, hold.data_ptr() + in_pad


def gpu_rgb_u8_to_yuv(rgb, chroma, cfg, pad=16, in_pad=0):
    """tg_rgb_u8_to_yuv_planar through the C ABI on (n,H,W,3) uint8 numpy -> (n, frame_bytes) uint8 numpy."""
    from tecogan_pytorch_amd import _lib as L
    n, H, W, _ = rgb.shape
    hold, src = _placed(rgb, in_pad)
    buf, out = _guarded(n * P.frame_bytes(H, W, chroma), pad, torch.uint8)
    c, m, r, s = _codes(chroma, *cfg)
    L.check(L.lib().tg_rgb_u8_to_yuv_planar(src, out.data_ptr(), n, H, W, c, m, r, s, _stream()), 'tg_rgb_u8_to_yuv_planar')
    torch.cuda.synchronize()
    assert _guards_intact(buf, pad), 'tg_rgb_u8_to_yuv_planar wrote outside its output'
    return out.cpu().numpy().reshape(n, -1)


def gpu_rgb_f32_to_yuv(rgb, chroma, depth, cfg, pad=16, in_pad=0):
    """tg_rgb_f32_to_yuv_planar16 through the C ABI on (n,3,H,W) float32 numpy -> (n, frame_samples) uint16 numpy."""
    from tecogan_pytorch_amd import _lib as L
    n, _, H, W = rgb.shape
    hold, src = _placed(rgb, in_pad)
    buf, out = _guarded(n * P.frame_bytes(H, W, chroma, depth), pad, torch.uint16)
    c, m, r, s = _codes(chroma, *cfg)
    L.check(L.lib().tg_rgb_f32_to_yuv_planar16(src, out.data_ptr(), n, H, W, c, depth, m, r, s, _stream()),
            'tg_rgb_f32_to_yuv_planar16')
    torch.cuda.synchronize()
    assert _guards_intact(buf, pad), 'tg_rgb_f32_to_yuv_planar16 wrote outside its output'
    return out.cpu().numpy().reshape(n, -1)


def gpu_yuv_to_rgb(yuv, h, w, chroma, depth, cfg, pad=16, in_pad=0):
    """tg_yuv_planar_to_rgb_f32 through the C ABI on (n, frame_samples) uint8 / uint16 numpy -> (n,3,h,w) float32."""
    from tecogan_pytorch_amd import _lib as L
    n = yuv.shape[0]
    assert yuv.dtype == (np.uint8 if depth == 8 else np.uint16) and yuv.shape[1] == P.frame_samples(h, w, chroma)
    hold, src = _placed(yuv, in_pad)
    buf, out = _guarded(n * 3 * h * w * 4, pad, torch.float32)
    c, m, r, s = _codes(chroma, *cfg)
    L.check(L.lib().tg_yuv_planar_to_rgb_f32(src, out.data_ptr(), n, h, w, c, depth, m, r, s, _stream()),
            'tg_yuv_planar_to_rgb_f32')
    torch.cuda.synchronize()
    assert _guards_intact(buf, pad), 'tg_yuv_planar_to_rgb_f32 wrote outside its output'
    return out.cpu().numpy().reshape(n, 3, h, w)


# ------------------------------------------------------------------ the two output directions: identity
def _rgb_u8_inputs(n, H, W, seed):
    rng = np.random.default_rng(seed)
    rnd = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    rnd[:, :, 0] = 255 - rnd[:, :, min(1, W - 1)]                   # the left column differs from its neighbour
    prim = rng.choice(np.array([0, 255], np.uint8), (n, H, W, 3))   # saturated primaries: the chroma clip at full range
    prim[0, 0, 0] = (0, 0, 255)
    prim[0, -1, -1] = (255, 0, 0)
    return {'random': rnd, 'primaries': prim}


def _rgb_f32_inputs(n, H, W, seed):
    x = _rgb_f32_input(n, H, W, seed)                               # below 0, above 1, NaN, infinities, the ties
    assert np.isnan(x).any() and (x < 0).any() and (x > 1).any()
    rng = np.random.default_rng(seed + 1)
    prim = rng.choice(np.array([0.0, 1.0], np.float32), (n, 3, H, W))
    prim[0, :, 0, 0] = (0, 0, 1)
    prim[0, :, -1, -1] = (1, 0, 0)
    return {'random': x, 'primaries': prim}


def _cfgs_of(chroma, H, W):
    """All sitings, matrices and ranges at the layout's two smallest shapes, one configuration at the rest."""
    return ALL_CFGS if (H, W) in OUT_SHAPES[chroma][:2] else [ONE_CFG[chroma]]


@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('chroma,H,W', OUT_CASES)
def test_rgb_u8_to_yuv_equals_the_specification_byte_for_byte(chroma, H, W, n):
    inputs = _rgb_u8_inputs(n, H, W, seed=H * 1000 + W + n)
    for cfg in _cfgs_of(chroma, H, W):
        for name, rgb in inputs.items():
            ref = P.rgb_u8_to_yuv(rgb, chroma, *cfg)
            got = gpu_rgb_u8_to_yuv(rgb, chroma, cfg)
            assert got.shape == ref.shape and np.array_equal(got, ref), (cfg, name, int((got != ref).sum()))
    for siting in P.SITINGS:                                        # pure blue / red reach chroma 256 before the clip
        blue = np.zeros((n, H, W, 3), np.uint8)
        blue[..., 2] = 255
        got = gpu_rgb_u8_to_yuv(blue, chroma, ('bt2020', True, siting))
        assert (P.planes(got, H, W, chroma)[1] == 255).all()
        assert (P.planes(gpu_rgb_u8_to_yuv(blue[..., ::-1], chroma, ('bt2020', True, siting)), H, W, chroma)[2] == 255).all()


@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('chroma,H,W', OUT_CASES)
def test_rgb_f32_to_yuv_equals_the_specification_word_for_word(chroma, H, W, n):
    inputs = _rgb_f32_inputs(n, H, W, seed=H * 1000 + W + n)
    for depth in (10, 12):
        top = (1 << depth) - 1
        for cfg in _cfgs_of(chroma, H, W):
            for name, rgb in inputs.items():
                ref = P.rgb_f32_to_yuv(rgb, chroma, depth, *cfg)
                assert ref.max() <= top
                got = gpu_rgb_f32_to_yuv(rgb, chroma, depth, cfg)
                assert got.shape == ref.shape and np.array_equal(got, ref), (depth, cfg, name, int((got != ref).sum()))
        blue = np.zeros((n, 3, H, W), np.float32)
        blue[:, 2] = 1.0
        for siting in P.SITINGS:
            got = gpu_rgb_f32_to_yuv(blue, chroma, depth, ('bt2020', True, siting))
            assert (P.planes(got, H, W, chroma)[1] == top).all()


@pytest.mark.parametrize('chroma', P.CHROMAS)
def test_both_output_directions_over_more_than_one_block(chroma):
    """n = 3 at 34x40: 1020 strips (510 at 4:2:0), several blocks of 256 threads, the last one partly idle."""
    n, H, W = 3, 34, 40
    for siting in P.SITINGS:
        cfg = ('bt2020', siting == 'left', siting)
        rgb = _rgb_u8_inputs(n, H, W, seed=7)['random']
        assert np.array_equal(gpu_rgb_u8_to_yuv(rgb, chroma, cfg), P.rgb_u8_to_yuv(rgb, chroma, *cfg))
        x = _rgb_f32_inputs(n, H, W, seed=8)['random']
        assert np.array_equal(gpu_rgb_f32_to_yuv(x, chroma, 10, cfg), P.rgb_f32_to_yuv(x, chroma, 10, *cfg))
        yuv = np.random.default_rng(9).integers(0, 256, (n, P.frame_samples(H, W, chroma)), dtype=np.uint8)
        err = np.abs(gpu_yuv_to_rgb(yuv, H, W, chroma, 8, cfg).astype(np.float64) - P.yuv_to_rgb(yuv, H, W, chroma, 8, *cfg)).max()
        assert err <= TOL[cfg[0]]


@pytest.mark.parametrize('chroma', P.CHROMAS)
def test_a_base_one_sample_off_its_wide_alignment_takes_the_element_wide_form(chroma):
    """W % 4 == 0 and, once per function, the output or the input one sample off: the same bytes, guards intact."""
    n, H, W = 2, 6, 8
    cfg = ('bt709', False, 'left')
    rgb = _rgb_u8_inputs(n, H, W, seed=3)['random']
    ref = P.rgb_u8_to_yuv(rgb, chroma, *cfg)
    assert np.array_equal(gpu_rgb_u8_to_yuv(rgb, chroma, cfg, pad=17), ref)          # the output one byte off a dword
    assert np.array_equal(gpu_rgb_u8_to_yuv(rgb, chroma, cfg, in_pad=1), ref)        # the input
    x = _rgb_f32_inputs(n, H, W, seed=4)['random']
    ref = P.rgb_f32_to_yuv(x, chroma, 12, *cfg)
    assert np.array_equal(gpu_rgb_f32_to_yuv(x, chroma, 12, cfg, pad=18), ref)       # the output one sample off 8 bytes
    assert np.array_equal(gpu_rgb_f32_to_yuv(x, chroma, 12, cfg, in_pad=4), ref)     # the input one float off 16 bytes
    rng = np.random.default_rng(5)
    for depth, one in ((8, 1), (10, 2)):
        yuv = rng.integers(0, 1 << depth, (n, P.frame_samples(H, W, chroma))).astype(np.uint8 if depth == 8 else np.uint16)
        wide = gpu_yuv_to_rgb(yuv, H, W, chroma, depth, cfg)
        assert np.array_equal(gpu_yuv_to_rgb(yuv, H, W, chroma, depth, cfg, in_pad=one), wide)      # the input one sample off
        assert np.array_equal(gpu_yuv_to_rgb(yuv, H, W, chroma, depth, cfg, pad=20), wide)          # the output one float off


# ------------------------------------------------------------------ the input direction
def _yuv_inputs(n, h, w, chroma, depth, seed):
    rng = np.random.default_rng(seed)
    ns, top = P.frame_samples(h, w, chroma), (1 << depth) - 1
    dt = np.uint8 if depth == 8 else np.uint16
    ch, cw = P.chroma_size(h, w, chroma)

    def const(y, u, v):
        one = np.concatenate([np.full(h * w, y), np.full(ch * cw, u), np.full(ch * cw, v)]).astype(dt)
        return np.broadcast_to(one, (n, ns)).copy()
    out = {'random': rng.integers(0, top + 1, (n, ns)).astype(dt), 'out_of_gamut': const(top, 0, top),
           'below_black': const(0, top, 0)}
    if depth > 8:                                                   # a share of the samples above 2^d - 1
        over = out['random'].copy()
        hit = rng.random((n, ns)) < 0.3
        hit[:, 0] = hit[:, -1] = True                               # (a luma and a chroma sample at the least)
        over[hit] = rng.integers(top + 1, 65536, int(hit.sum()), dtype=np.uint16)
        out['above_top'] = over
    return out


@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('depth', P.DEPTHS)
@pytest.mark.parametrize('h,w', [(2, 2), (3, 5), (9, 11), (16, 24)])
def test_yuv_to_rgb_is_within_the_derived_bound_of_fp64_and_inside_the_unit_range(h, w, depth, n):
    worst = dict.fromkeys(TOL, 0.0)
    for chroma in P.CHROMAS:
        inputs = _yuv_inputs(n, h, w, chroma, depth, seed=h * 1000 + w + n + depth)
        assert depth == 8 or (inputs['above_top'] > (1 << depth) - 1).any()
        for cfg in ALL_CFGS:
            for name, yuv in inputs.items():
                ref = P.yuv_to_rgb(yuv, h, w, chroma, depth, *cfg)
                got = gpu_yuv_to_rgb(yuv, h, w, chroma, depth, cfg)           # (16,24) aligned: the wide form
                assert got.dtype == np.float32 and got.shape == ref.shape
                assert got.min() >= 0.0 and got.max() <= 1.0, (chroma, cfg, name)
                err = float(np.abs(got.astype(np.float64) - ref).max())
                worst[cfg[0]] = max(worst[cfg[0]], err)
                assert err <= TOL[cfg[0]], (chroma, cfg, name, err)
            assert (gpu_yuv_to_rgb(inputs['out_of_gamut'], h, w, chroma, depth, cfg)[:, 0] == 1.0).all()
        if depth > 8:                                               # a sample above the top code is the top code, bit for bit
            clipped = np.minimum(inputs['above_top'], (1 << depth) - 1).astype(np.uint16)
            cfg = ONE_CFG[chroma]
            assert np.array_equal(gpu_yuv_to_rgb(inputs['above_top'], h, w, chroma, depth, cfg),
                                  gpu_yuv_to_rgb(clipped, h, w, chroma, depth, cfg))
    print('worst |gpu - fp64| at %dx%d n=%d depth %d: %s (bounds %s)'
          % (h, w, n, depth, {k: '%.3g' % v for k, v in worst.items()}, TOL))


# ------------------------------------------------------------------ 4:2:0 with BT.601 / BT.709: the four existing kernels
@pytest.mark.parametrize('H,W', [(2, 2), (4, 6), (6, 8), (18, 22), (16, 24)])
def test_420_instantiations_equal_the_four_existing_entry_points_bit_for_bit(H, W):
    from tecogan_pytorch_amd import _lib as L
    from tests.test_hip_yuv import gpu_rgb_to_yuv420, gpu_yuv420_to_rgb
    from tests.test_hip_yuv_depth import gpu_rgb_f32_to_yuv420p, gpu_yuv420p_to_rgb
    n = 3
    rgb = _rgb_u8_inputs(n, H, W, seed=H + W)['random']
    x = _rgb_f32_inputs(n, H, W, seed=H * W)['random']
    rng = np.random.default_rng(H * W)
    for siting in R8.SITINGS:
        for matrix, full in R8.CONFIGS:
            cfg = (matrix, full, siting)
            assert np.array_equal(gpu_rgb_u8_to_yuv(rgb, '420', cfg), gpu_rgb_to_yuv420(rgb, cfg))
            for depth in (10, 12):
                assert np.array_equal(gpu_rgb_f32_to_yuv(x, '420', depth, cfg),
                                      gpu_rgb_f32_to_yuv420p(torch.from_numpy(x).to(DEV), depth, cfg))
            for h, w in ((H, W), (H + 1, W + 3)):                   # the way in takes odd sizes as well
                y8 = rng.integers(0, 256, (n, P.frame_samples(h, w, '420')), dtype=np.uint8)
                assert np.array_equal(gpu_yuv_to_rgb(y8, h, w, '420', 8, cfg), gpu_yuv420_to_rgb(y8, h, w, cfg))
                y16 = rng.integers(0, 65536, (n, P.frame_samples(h, w, '420')), dtype=np.uint16)
                for depth in (10, 12):
                    assert np.array_equal(gpu_yuv_to_rgb(y16, h, w, '420', depth, cfg), gpu_yuv420p_to_rgb(y16, h, w, depth, cfg))


# ------------------------------------------------------------------ refusals and the ops wrappers
def test_entry_points_return_tg_e_arg_without_a_launch_and_the_old_ones_still_refuse_bt2020():
    from tecogan_pytorch_amd import _lib as L
    lib = L.lib()
    rgb = torch.full((3 * 6 * 6,), 7.0, device=DEV)
    u8 = torch.full((3 * 6 * 6 + 4,), 9, dtype=torch.uint8, device=DEV)
    yuv = torch.full((2 * P.frame_samples(6, 6, '444') + 8,), GUARD, dtype=torch.uint8, device=DEV)
    st = _stream()
    fin, out8, out16 = lib.tg_yuv_planar_to_rgb_f32, lib.tg_rgb_u8_to_yuv_planar, lib.tg_rgb_f32_to_yuv_planar16
    R, U, Y = rgb.data_ptr(), u8.data_ptr(), yuv.data_ptr()
    for chroma in (3, -1, 420):
        assert fin(Y, R, 1, 6, 6, chroma, 8, 1, 0, 1, st) == E_ARG
        assert b'chroma' in lib.tg_last_error_string()
        assert out8(U, Y, 1, 6, 6, chroma, 1, 0, 1, st) == E_ARG
        assert out16(R, Y, 1, 6, 6, chroma, 10, 1, 0, 1, st) == E_ARG
    for depth in (9, 11, 14, 16, 0, -8):
        assert fin(Y, R, 1, 6, 6, 1, depth, 1, 0, 1, st) == E_ARG
        assert b'depth' in lib.tg_last_error_string()
        assert out16(R, Y, 1, 6, 6, 1, depth, 1, 0, 1, st) == E_ARG
    assert out16(R, Y, 1, 6, 6, 1, 8, 1, 0, 1, st) == E_ARG                                     # (8 bits are the other function's)
    for m, r, s in ((3, 0, 0), (-1, 0, 0), (0, 2, 0), (0, 0, 2)):
        assert fin(Y, R, 1, 6, 6, 2, 8, m, r, s, st) == E_ARG
        assert out8(U, Y, 1, 6, 6, 2, m, r, s, st) == E_ARG
        assert out16(R, Y, 1, 6, 6, 2, 12, m, r, s, st) == E_ARG
    for H, W, chroma in ((6, 5, 1), (5, 6, 0), (6, 5, 0)):                                      # odd W at 4:2:2, odd H / W at 4:2:0
        assert out8(U, Y, 1, H, W, chroma, 1, 0, 1, st) == E_ARG
        assert b'even' in lib.tg_last_error_string()
        assert out16(R, Y, 1, H, W, chroma, 10, 1, 0, 1, st) == E_ARG
    assert fin(Y, R, 1, 1, 6, 2, 8, 1, 0, 1, st) == E_ARG and fin(Y, R, 0, 6, 6, 2, 8, 1, 0, 1, st) == E_ARG
    assert out8(U, Y, 0, 6, 6, 2, 1, 0, 1, st) == E_ARG and out16(R, Y, 0, 6, 6, 2, 10, 1, 0, 1, st) == E_ARG
    for call in (lambda: fin(None, R, 1, 6, 6, 2, 8, 1, 0, 1, st), lambda: fin(Y, None, 1, 6, 6, 2, 8, 1, 0, 1, st),
                 lambda: out8(None, Y, 1, 6, 6, 2, 1, 0, 1, st), lambda: out8(U, None, 1, 6, 6, 2, 1, 0, 1, st),
                 lambda: out16(None, Y, 1, 6, 6, 2, 10, 1, 0, 1, st), lambda: out16(R, None, 1, 6, 6, 2, 10, 1, 0, 1, st)):
        assert call() == E_ARG
        assert b'null' in lib.tg_last_error_string()
    assert fin(Y + 1, R, 1, 6, 6, 2, 10, 1, 0, 1, st) == E_ARG                                  # 16-bit samples on an odd byte
    assert b'aligned' in lib.tg_last_error_string()
    assert fin(Y, R + 2, 1, 6, 6, 2, 8, 1, 0, 1, st) == E_ARG                                   # an fp32 pointer off a float
    assert out16(R, Y + 1, 1, 6, 6, 2, 10, 1, 0, 1, st) == E_ARG and out16(R + 1, Y, 1, 6, 6, 2, 10, 1, 0, 1, st) == E_ARG
    # the four existing functions keep their two matrices
    assert lib.tg_yuv420_to_rgb_f32(Y, R, 1, 6, 6, 2, 0, 1, st) == E_ARG
    assert lib.tg_rgb_u8_to_yuv420(U, Y, 1, 6, 6, 2, 0, 1, st) == E_ARG
    assert lib.tg_yuv420p16_to_rgb_f32(Y, R, 1, 6, 6, 10, 2, 0, 1, st) == E_ARG
    assert lib.tg_rgb_f32_to_yuv420p16(R, Y, 1, 6, 6, 10, 2, 0, 1, st) == E_ARG
    torch.cuda.synchronize()
    assert bool((yuv == GUARD).all()) and bool((rgb == 7.0).all()) and bool((u8 == 9).all()), 'a refused call launched'


def test_ops_wrappers_equal_the_c_abi_and_refuse_bad_arguments():
    from tecogan_pytorch_amd import _lib as L, ops
    rgb = _rgb_u8_inputs(2, 5, 10, seed=1)['random']
    x = _rgb_f32_inputs(2, 5, 10, seed=2)['random']
    dev8, devf = torch.from_numpy(rgb).to(DEV), torch.from_numpy(x).to(DEV)
    for chroma, cfg in (('422', ('bt2020', False, 'left')), ('444', ('bt601', True, 'center'))):
        got = ops.rgb_to_yuv(dev8, chroma, *cfg)
        assert got.dtype == torch.uint8 and got.shape == (2, ops.yuv_frame_samples(5, 10, chroma)) == (2, P.frame_samples(5, 10, chroma))
        assert np.array_equal(got.cpu().numpy(), P.rgb_u8_to_yuv(rgb, chroma, *cfg))
        deep = ops.rgb_f32_to_yuv(devf, chroma, 12, *cfg)
        assert deep.dtype == torch.uint16 and np.array_equal(deep.cpu().numpy(), P.rgb_f32_to_yuv(x, chroma, 12, *cfg))
        into = torch.zeros_like(deep)
        assert ops.rgb_f32_to_yuv(devf, chroma, 12, *cfg, out=into) is into and torch.equal(into.view(torch.uint8), deep.view(torch.uint8))
        back = ops.yuv_to_rgb(got, 5, 10, chroma, 8, *cfg)
        assert back.shape == (2, 3, 5, 10) and np.array_equal(back.cpu().numpy(), gpu_yuv_to_rgb(got.cpu().numpy(), 5, 10, chroma, 8, cfg))
        assert torch.equal(ops.yuv_to_rgb(got[0], 5, 10, chroma, 8, *cfg), back[:1])
        back12 = ops.yuv_to_rgb(deep, 5, 10, chroma, 12, *cfg)
        assert np.array_equal(back12.cpu().numpy(), gpu_yuv_to_rgb(deep.cpu().numpy(), 5, 10, chroma, 12, cfg))
        into = torch.zeros_like(back12)
        assert ops.yuv_to_rgb(deep, 5, 10, chroma, 12, *cfg, out=into) is into and torch.equal(into, back12)
    for bad in (lambda: ops.rgb_to_yuv(torch.from_numpy(rgb)), lambda: ops.rgb_to_yuv(dev8, '411'),
                lambda: ops.rgb_to_yuv(dev8, '444', matrix='bt2100'), lambda: ops.yuv_to_rgb(dev8.view(2, -1), 5, 10, '420'),
                lambda: ops.yuv_to_rgb(ops.rgb_to_yuv(dev8, '444'), 5, 10, '444', 10),               # bytes are not samples
                lambda: ops.rgb_f32_to_yuv(devf, '444', 10, out=torch.zeros(2, 5, dtype=torch.uint16, device=DEV))):
        with pytest.raises(L.TecoganHipError):
            bad()
    with pytest.raises(L.TecoganHipError, match='code -2'):
        ops.rgb_to_yuv(dev8[:, :, :9].contiguous(), '422')          # an odd width
    with pytest.raises(L.TecoganHipError, match='code -2'):
        ops.rgb_f32_to_yuv(devf, '444', 8)
    with pytest.raises(L.TecoganHipError):
        ops.rgb_to_yuv420(dev8[:, :4].contiguous(), matrix='bt2020')                 # the old wrappers are unchanged


# ------------------------------------------------------------------ the stream
@pytest.fixture(scope='module')
def net4():
    return make_net('BD', 4)


def planar_clip(t, h, w, chroma, depth, seed, cfg):
    """(t, frame_bytes) uint8: the bytes of a smooth moving clip in the layout `chroma` at `depth` bits -- the float clip
    converted by the numpy specification at the size that covers h x w in whole chroma samples, its Y plane cropped."""
    sx, sy = P.SUB[chroma]
    he, we = sy * ((h + sy - 1) // sy), sx * ((w + sx - 1) // sx)
    clip = smooth_clip(t, 3, he, we, seed=seed)
    if depth == 8:
        u8 = (clip.permute(0, 2, 3, 1) * 255.0).round().clamp(0, 255).to(torch.uint8).numpy()
        full = P.rgb_u8_to_yuv(u8, chroma, *cfg)
    else:
        full = P.rgb_f32_to_yuv(clip.numpy().astype(np.float32), chroma, depth, *cfg)
    y, u, v = P.planes(full, he, we, chroma)
    out = np.ascontiguousarray(np.concatenate([y[:, :h, :w].reshape(t, -1), u.reshape(t, -1), v.reshape(t, -1)], 1))
    assert out.shape[1] == P.frame_samples(h, w, chroma)
    return out.view(np.uint8)


def streamed(net, items, spec, ofb=None, **kw):
    out = [c.copy() for c in net.infer_stream(iter(items), DEV, yuv=spec, **kw)]
    ofb = spec.out_frame_bytes(net.scale) if ofb is None else ofb
    assert all(c.dtype == np.uint8 and c.ndim == 2 and c.shape[1] == ofb for c in out)
    return np.concatenate(out, 0) if out else np.zeros((0, ofb), np.uint8)


def lr_frames(clip, spec):
    """The LR frames of the clip's bytes: ops.yuv_to_rgb, (t,3,h,w) on the device."""
    from tecogan_pytorch_amd import ops
    dev = torch.from_numpy(clip if spec.depth == 8 else clip.view(np.uint16)).to(DEV)
    return ops.yuv_to_rgb(dev, spec.h, spec.w, spec.chroma, spec.depth, spec.matrix, spec.full_range, spec.siting)


def reference(net, clip, spec, cuts=(), resize=None):
    """What the stream must yield, from the ops alone.  8-bit output: ops.rgb_to_yuv of the RGB chunks a stream WITHOUT
    `yuv` yields when it is fed ops.yuv_to_rgb of the same frames.  Deep output: ops.rgb_f32_to_yuv of the float HR
    frames (test_hip_yuv_depth.float_frames; a forced cut starts a clip of its own)."""
    from tecogan_pytorch_amd import ops
    from tecogan_pytorch_amd.models.networks import SceneCut
    lr = lr_frames(clip, spec)
    cfg = (spec.matrix, spec.full_range, spec.siting)
    if spec.od == 8:
        kw = {} if not cuts else {'scene_cut': SceneCut(at=cuts)}
        if resize is not None:
            kw['resize'] = resize
        rgb = np.concatenate([c.copy() for c in net.infer_stream(iter([lr]), DEV, **kw)], 0)
        return ops.rgb_to_yuv(torch.from_numpy(rgb).to(DEV), spec.oc, *cfg).cpu().numpy()
    edges = [0] + list(cuts) + [len(clip)]
    hr = torch.cat([float_frames(net, lr[a:b]) for a, b in zip(edges[:-1], edges[1:])], 0)
    return ops.rgb_f32_to_yuv(hr, spec.oc, spec.od, *cfg).cpu().numpy().view(np.uint8)


CONVERSIONS = {                                      # chroma, out_chroma, depth, out_depth, (matrix, full, siting)
    '420_to_444': ('420', '444', 8, None, ('bt709', False, 'left')),
    '422p10_to_422p10': ('422', None, 10, None, ('bt2020', False, 'left')),
    '444_to_420': ('444', '420', 8, None, ('bt601', True, 'center')),
    '444_to_444p12': ('444', None, 8, 12, ('bt2020', True, 'center')),
}


@pytest.mark.parametrize('t', [1, 10])
@pytest.mark.parametrize('h,w', [(16, 24), (9, 11)])
@pytest.mark.parametrize('conv', sorted(CONVERSIONS))
def test_stream_equals_the_ops_bit_for_bit(net4, conv, h, w, t):
    from tecogan_pytorch_amd.models.networks import Yuv, yuv_planes
    chroma, oc, depth, od, cfg = CONVERSIONS[conv]
    spec = Yuv(h, w, chroma, oc, *cfg, depth=depth, out_depth=od)
    clip = planar_clip(t, h, w, chroma, depth, 40 + t, cfg)
    assert clip.shape == (t, spec.frame_bytes)
    ref = reference(net4, clip, spec)
    assert ref.shape == (t, spec.out_frame_bytes(4)) == (t, P.frame_bytes(4 * h, 4 * w, spec.oc, spec.od))
    for name, items in chunkings(clip).items():
        got = streamed(net4, items, spec)
        assert got.shape == ref.shape and np.array_equal(got, ref), (name, int((got != ref).sum()))
    y, u, v = yuv_planes(got, 4 * h, 4 * w, spec.oc, spec.od)
    ch, cw = P.chroma_size(4 * h, 4 * w, spec.oc)
    assert y.shape == (t, 4 * h, 4 * w) and u.shape == v.shape == (t, ch, cw)
    assert y.dtype == (np.uint8 if spec.od == 8 else np.uint16) and int(max(y.max(), u.max(), v.max())) <= (1 << spec.od) - 1
    if depth > 8 and t == 10:                                       # samples in place of bytes: the same stream
        assert np.array_equal(streamed(net4, [clip.view(np.uint16)], spec), ref)


def test_stream_with_a_forced_scene_cut(net4):
    from tecogan_pytorch_amd.models.networks import SceneCut, Yuv
    cfg = ('bt2020', False, 'left')
    spec = Yuv(16, 24, '422', '444', *cfg, depth=10, out_depth=10)
    clip = planar_clip(13, 16, 24, '422', 10, 12, cfg)
    sc = SceneCut(at=(4,))
    got = streamed(net4, chunkings(clip)['frames'], spec, scene_cut=sc)
    assert sc.cuts == [4]
    assert np.array_equal(got, reference(net4, clip, spec, cuts=(4,)))
    assert not np.array_equal(got[4:], reference(net4, clip, spec)[4:])


@pytest.mark.parametrize('oc,rh,rw', [('422', 45, 70), ('444', 45, 71)])
def test_stream_with_a_resize_on_an_8_bit_output(net4, oc, rh, rw):
    """An odd height at 4:2:2, odd sides at 4:4:4: sizes an I420 output cannot have."""
    from tecogan_pytorch_amd.models.networks import Resize, Yuv
    cfg = ('bt709', False, 'center')
    spec = Yuv(9, 11, '420', oc, *cfg)
    clip = planar_clip(10, 9, 11, '420', 8, 6, cfg)
    got = streamed(net4, chunkings(clip)['uneven'], spec, ofb=P.frame_bytes(rh, rw, oc), resize=Resize(rh, rw))
    assert np.array_equal(got, reference(net4, clip, spec, resize=Resize(rh, rw)))


def test_resize_to_an_odd_width_is_refused_for_422_before_any_allocation(net4):
    from tecogan_pytorch_amd.models.networks import Resize, Yuv
    pulled = []

    def items():
        pulled.append(1)
        yield np.zeros(Yuv(16, 24).frame_bytes, np.uint8)
    before = torch.cuda.memory_allocated(DEV)
    with pytest.raises(ValueError, match='even width'):
        net4.infer_stream(items(), DEV, yuv=Yuv(16, 24, out_chroma='422'), resize=Resize(64, 95))
    with pytest.raises(ValueError, match='8-bit'):
        net4.infer_stream(items(), DEV, yuv=Yuv(16, 24, out_chroma='444', out_depth=10), resize=Resize(64, 96))
    assert pulled == [] and torch.cuda.memory_allocated(DEV) == before
    assert streamed(net4, [], Yuv(16, 24, out_chroma='422'), ofb=64 * 96 * 2, resize=Resize(64, 96)).shape[0] == 0


def test_stream_2x_bi():
    from tecogan_pytorch_amd.models.networks import Yuv
    net = make_net('BI', 2)
    cfg = ('bt2020', True, 'left')
    spec = Yuv(9, 11, '444', '422', *cfg, depth=12, out_depth=10)
    clip = planar_clip(19, 9, 11, '444', 12, 8, cfg)
    ref = reference(net, clip, spec)
    assert ref.shape == (19, 2 * 2 * 18 * 22)
    assert np.array_equal(streamed(net, chunkings(clip)['uneven'], spec), ref)


# ------------------------------------------------------------------ the unchanged path
NEW = ('tg_yuv_planar_to_rgb_f32', 'tg_rgb_u8_to_yuv_planar', 'tg_rgb_f32_to_yuv_planar16')


def _recorded_stream(net, monkeypatch, items, spec):
    from tecogan_pytorch_amd import _lib as L
    rec = _Recorder(L.lib())
    with monkeypatch.context() as mp:
        mp.setattr(L, 'lib', lambda: rec)
        out = streamed(net, items, spec)
    return out, [c for c in rec.calls if c not in QUIET]


def test_a_yuv420_stream_calls_none_of_the_new_entry_points(net4, monkeypatch):
    """The launch list of a Yuv420 stream is the one test_hip_yuv_depth.py pins for a stream without this code: the same
    counts, none of the three new names; and a Yuv at '420' records the same list with the new names in their places."""
    from tecogan_pytorch_amd.models.networks import Yuv, Yuv420
    from tecogan_pytorch_amd.models.networks.frnet_infer import clip_batches, stream_batch_sizes
    from tests.test_hip_yuv_depth import deep_clip
    h, w, t = 16, 24, 21
    clip = deep_clip(t, h, w, 8, 3)
    frames = chunkings(clip)['frames']
    streamed(net4, frames, Yuv420(h, w))                           # plans of every batch size exist before recording
    got, kinds = _recorded_stream(net4, monkeypatch, frames, Yuv420(h, w))
    _, kinds_10 = _recorded_stream(net4, monkeypatch, frames, Yuv420(h, w, out_depth=10))
    assert not [k for k in kinds + kinds_10 if k in NEW]
    nb = len(clip_batches(t, *stream_batch_sizes()))
    assert kinds.count('tg_frnet_step_srnet') == t and kinds.count('tg_rgb_u8_to_yuv420') == nb
    assert kinds.count('tg_yuv420_to_rgb_f32') == nb and kinds.count('tg_frnet_step_phase') == nb
    assert kinds_10.count('tg_rgb_f32_to_yuv420p16') == t and 'tg_rgb_u8_to_yuv420' not in kinds_10
    assert [k for k in kinds_10 if k != 'tg_rgb_f32_to_yuv420p16'] == [k for k in kinds if k != 'tg_rgb_u8_to_yuv420']
    # a Yuv takes the new launches, one for one, and yields the same bytes at 4:2:0
    old_of = {'tg_yuv_planar_to_rgb_f32': 'tg_yuv420_to_rgb_f32', 'tg_rgb_u8_to_yuv_planar': 'tg_rgb_u8_to_yuv420',
              'tg_rgb_f32_to_yuv_planar16': 'tg_rgb_f32_to_yuv420p16'}
    got_p, kinds_p = _recorded_stream(net4, monkeypatch, frames, Yuv(h, w))
    assert np.array_equal(got_p, got)
    assert not [k for k in kinds_p if k in old_of.values()] and [old_of.get(k, k) for k in kinds_p] == kinds
    _, kinds_p10 = _recorded_stream(net4, monkeypatch, frames, Yuv(h, w, out_depth=10))
    assert [old_of.get(k, k) for k in kinds_p10] == kinds_10


# ------------------------------------------------------------------ the CLI
def test_cli_y4m_422p10_in_444p10_out(tmp_path):
    import yaml
    from tecogan_pytorch_amd import main as M
    from tecogan_pytorch_amd.data.y4m import Y4MReader
    from tecogan_pytorch_amd.models.networks import Yuv
    pth = str(tmp_path / 'G_iter7.pth')
    torch.save(generator_state_dict(scale=4, degradation='BD'), pth)
    opt = M.default_opt()
    opt['model']['generator']['load_path'] = pth
    yml = str(tmp_path / 'infer.yml')
    with open(yml, 'w') as f:
        yaml.safe_dump(opt, f)
    h, w, t = 16, 24, 12
    cfg = ('bt2020', False, 'center')
    clip = planar_clip(t, h, w, '422', 10, 31, cfg)
    src, dst = str(tmp_path / 'in.y4m'), str(tmp_path / 'out.y4m')
    with open(src, 'wb') as f:
        f.write(b'YUV4MPEG2 W24 H16 F25:1 Ip A1:1 C422p10 XYSCSS=422P10\n')
        for fr in clip:
            f.write(b'FRAME\n' + fr.tobytes())
    M.main(['--mode', 'infer', '--opt', yml, '--input', src, '--output', dst, '--yuv-matrix', 'bt2020', '--yuv-siting', 'center',
            '--output-chroma', '444'])
    rd = Y4MReader(io.BytesIO(open(dst, 'rb').read()), depths=(8, 10, 12), chromas=('420', '422', '444'))
    assert (rd.w, rd.h, rd.chroma, rd.depth, rd.siting, rd.full_range) == (96, 64, '444', 10, None, None)
    assert rd.header['tags'] == ['F25:1', 'A1:1', 'C444p10', 'XYSCSS=444P10']
    got = np.stack([fr.copy() for fr in rd])
    # the model wrapper pads the front; the engine on the padded clip is the reference, and that is the op's bytes
    n_pad = opt['test']['num_pad_front']
    assert opt['test'].get('padding_mode', 'reflect') == 'reflect' and 0 < n_pad < t
    net = make_net('BD', 4)
    spec = Yuv(h, w, '422', '444', *cfg, depth=10)
    padded = np.concatenate([clip[1:1 + n_pad][::-1], clip], 0)
    ref = reference(net, padded, spec)[n_pad:]
    assert got.shape == ref.shape == (t, spec.out_frame_bytes(4)) == (t, 2 * 3 * 64 * 96) and np.array_equal(got, ref)
