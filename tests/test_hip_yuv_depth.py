"""10- and 12-bit YUV 4:2:0 on the GPU: the two kernels through the C ABI against
tests/yuv_depth_ref.py -- fp32 RGB -> I420 at d bits WORD FOR WORD, I420 at d bits -> RGB within 3.5e-7 of fp64 -- at
shapes that take the wide and the element-wide form of either kernel, with guard bytes around every output; and
FRNet.infer_stream(yuv=Yuv420(..., depth, out_depth)) / the CLI, whose bytes equal ops.rgb_f32_to_yuv420p of the float HR
frames, which the test collects itself from enqueue_batch on its own ping-pong pair.

Tolerance of the input direction, 3.5e-7 absolute, derived as tests/test_hip_yuv.py derives its own, for 12-bit operands
(10-bit ones are smaller term by term).  Y - yo (at most 3839 in magnitude) and C16 - 16 mid (at most 32768) are exact
in fp32, the coefficients are fp64 values rounded once, and every rounding is at most 2^-24 = 5.96e-8 relative.
yf = ky (Y - yo): |yf| <= 3839/3504 = 1.0956 carries two roundings (ky, the product): 1.306e-7.  B = fma(bu, du, yf):
|bu du| <= 1.8556 * 2048/3584 = 1.0603 carries the rounding of bu, 6.32e-8, and the result, at most 2.156, the fma's
own, 1.285e-7: 3.22e-7 in all; R is smaller term by term.  G = fma(gv, dv, fma(gu, du, yf)) under BT.601, the larger
gains: 1.306e-7 (yf) + 1.17e-8 (gu, |gu du| <= 0.1966) + 7.70e-8 (inner result <= 1.292) + 2.43e-8 (gv, |gv dv| <=
0.408) + 1.013e-7 (outer result <= 1.700) = 3.45e-7.  Full range has |yf| <= 1 and |du|/cs <= 0.5001: smaller.  The clamp
adds nothing.  The bound used is the larger of the two sums, 3.45e-7, written as 3.5e-7."""
import io
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from procedural_weights import generator_state_dict, smooth_clip
from tests import yuv_depth_ref as R
from tests import yuv_ref as R8

DEV = torch.device('cuda', 0)
GUARD = 0xA5
TOL = 3.5e-7                                     # see the module docstring
E_ARG = -2


def _codes(matrix, full, siting):
    from tecogan_pytorch_amd import _lib as L
    return L.YUV_MATRIX[matrix], int(full), L.YUV_SITING[siting]


def _guarded(nbytes, pad, dtype):
    """A device buffer of `nbytes` payload bytes with `pad` guard bytes on either side, all set to GUARD; the payload
    starts `pad` bytes into a 256-byte aligned allocation (pad 16: aligned for every vector access; pad 18: two bytes
    off a 16-byte boundary, aligned for 2-byte stores only)."""
    buf = torch.full((pad + nbytes + pad,), GUARD, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 256 == 0
    return buf, buf[pad:pad + nbytes].view(dtype)


def _guards_intact(buf, pad):
    return bool((buf[:pad] == GUARD).all()) and bool((buf[-pad:] == GUARD).all())


def gpu_rgb_f32_to_yuv420p(rgb, depth, cfg, pad=16):
    """tg_rgb_f32_to_yuv420p16 through the C ABI on a (n,3,H,W) float32 DEVICE tensor -> (n, frame_samples) uint16."""
    from tecogan_pytorch_amd import _lib as L
    n, _, H, W = rgb.shape
    buf, out = _guarded(n * R.frame_bytes(H, W), pad, torch.uint16)
    L.check(L.lib().tg_rgb_f32_to_yuv420p16(rgb.data_ptr(), out.data_ptr(), n, H, W, depth, *_codes(*cfg),
                                            torch.cuda.current_stream().cuda_stream), 'tg_rgb_f32_to_yuv420p16')
    torch.cuda.synchronize()
    assert _guards_intact(buf, pad), 'tg_rgb_f32_to_yuv420p16 wrote outside its output'
    return out.cpu().numpy().reshape(n, -1)


def gpu_yuv420p_to_rgb(yuv, h, w, depth, cfg, pad=16, in_pad=0):
    """tg_yuv420p16_to_rgb_f32 through the C ABI on (n, frame_samples) uint16 numpy -> (n,3,h,w) float32 numpy; the
    input sits in_pad bytes (an even number) into its buffer."""
    from tecogan_pytorch_amd import _lib as L
    n = yuv.shape[0]
    src = torch.empty(in_pad + 2 * yuv.size, dtype=torch.uint8, device=DEV)
    src[in_pad:].copy_(torch.from_numpy(np.ascontiguousarray(yuv).view(np.uint8).reshape(-1)))
    buf, out = _guarded(n * 3 * h * w * 4, pad, torch.float32)
    L.check(L.lib().tg_yuv420p16_to_rgb_f32(src.data_ptr() + in_pad, out.data_ptr(), n, h, w, depth, *_codes(*cfg),
                                            torch.cuda.current_stream().cuda_stream), 'tg_yuv420p16_to_rgb_f32')
    torch.cuda.synchronize()
    assert _guards_intact(buf, pad), 'tg_yuv420p16_to_rgb_f32 wrote outside its output'
    return out.cpu().numpy().reshape(n, 3, h, w)


# ------------------------------------------------------------------ fp32 RGB -> I420 at d bits: word identity
def _rgb_f32_input(n, H, W, seed):
    """Uniform in [-0.25, 1.25] with, scattered over it: exact 0 and 1, NaN, both infinities, values whose fp32 product
    with 65535 is k + 0.5 exactly (the ties of the one float step), and a left column unlike its neighbour."""
    rng = np.random.default_rng(seed)
    x = (rng.random((n, 3, H, W), dtype=np.float32) * np.float32(1.5) - np.float32(0.25)).astype(np.float32)
    ties = ((np.arange(0, 65535, dtype=np.float64) + 0.5) / 65535.0).astype(np.float32)
    prod = ties * np.float32(65535.0)
    ties = ties[prod == np.floor(prod) + np.float32(0.5)]
    assert ties.size > 1000
    flat = x.reshape(-1)
    special = np.concatenate([rng.choice(ties, max(4, flat.size // 4)),
                              np.array([0.0, 1.0, -0.0, np.nan, np.inf, -np.inf, 2.0, -3.0, 0.5], np.float32)])
    at = rng.choice(flat.size, min(flat.size, special.size), replace=False)
    flat[at] = special[:at.size]
    x[:, :, :, 0] = np.float32(1.0) - x[:, :, :, 1]
    x[0, 0, 0, 0] = np.nan
    return x


@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('H,W', [(2, 2), (4, 6), (18, 22), (64, 130), (6, 8), (64, 96)])
def test_rgb_f32_to_yuv420p_equals_the_specification_word_for_word(H, W, n):
    """(6,8) and (64,96) take the wide form at the aligned placement (W a multiple of 4); every shape takes the
    element-wide form two bytes off a 16-byte boundary."""
    x = _rgb_f32_input(n, H, W, seed=H * 1000 + W + n)
    assert np.isnan(x).any() and (x < 0).any() and (x > 1).any()
    dev = torch.from_numpy(x).to(DEV)
    for depth, siting, matrix, full in R.CASES:
        ref = R.rgb_f32_to_yuv420p(x, depth, matrix, full, siting)
        assert ref.max() <= (1 << depth) - 1
        for pad in (16, 18):
            got = gpu_rgb_f32_to_yuv420p(dev, depth, (matrix, full, siting), pad=pad)
            assert got.shape == ref.shape and np.array_equal(got, ref), \
                (depth, siting, matrix, full, pad, int((got != ref).sum()))


def test_rgb_f32_to_yuv420p_input_off_a_16_byte_boundary():
    """The fp32 input 4 bytes into its allocation: the element-wide loads, whatever the width."""
    x = _rgb_f32_input(2, 16, 24, seed=9)
    hold = torch.empty(x.size + 1, dtype=torch.float32, device=DEV)
    hold[1:].copy_(torch.from_numpy(x).reshape(-1))
    dev = hold[1:].view(2, 3, 16, 24)
    assert dev.data_ptr() % 16 == 4
    for depth, siting, matrix, full in R.CASES[::3]:
        assert np.array_equal(gpu_rgb_f32_to_yuv420p(dev, depth, (matrix, full, siting)),
                              R.rgb_f32_to_yuv420p(x, depth, matrix, full, siting))


def test_full_range_chroma_reaches_the_clip():
    """Pure blue and red give chroma 2^d - 0.5 before the clip in full range: the top code, not 2^d."""
    for depth in R.DEPTHS:
        top = (1 << depth) - 1
        for c, plane in ((2, 1), (0, 2)):
            x = np.zeros((1, 3, 4, 8), np.float32)
            x[:, c] = 1.0
            for siting in R.SITINGS:
                got = gpu_rgb_f32_to_yuv420p(torch.from_numpy(x).to(DEV), depth, ('bt709', True, siting))
                assert (R.planes(got, 4, 8)[plane] == top).all()


# ------------------------------------------------------------------ I420 at d bits -> fp32 RGB
def _yuv16_inputs(n, h, w, depth, seed):
    rng = np.random.default_rng(seed)
    ns, top = R.frame_samples(h, w), (1 << depth) - 1
    ch, cw = (h + 1) // 2, (w + 1) // 2

    def const(y, u, v):
        one = np.concatenate([np.full(h * w, y), np.full(ch * cw, u), np.full(ch * cw, v)]).astype(np.uint16)
        return np.broadcast_to(one, (n, ns)).copy()
    rnd = rng.integers(0, top + 1, (n, ns), dtype=np.uint16)
    over = rnd.copy()                                               # a share of the samples above 2^d - 1
    hit = rng.random((n, ns)) < 0.3
    over[hit] = rng.integers(top + 1, 65536, int(hit.sum()), dtype=np.uint16)
    return {'random': rnd, 'above_top': over, 'all_ones': np.full((n, ns), 65535, np.uint16),
            'out_of_gamut': const(top, 0, top), 'out_of_gamut_mirror': const(top, top, 0),
            'below_black': const(0, top, 0), 'below_black_mirror': const(0, 0, top)}


@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('h,w', [(2, 2), (3, 5), (9, 11), (16, 24), (4, 6), (6, 8)])
def test_yuv420p_to_rgb_is_within_the_derived_bound_of_fp64_and_inside_the_unit_range(h, w, n):
    worst = 0.0
    for depth, siting, matrix, full in R.CASES:
        cfg = (matrix, full, siting)
        inputs = _yuv16_inputs(n, h, w, depth, seed=h * 1000 + w + n + depth)
        assert (inputs['above_top'] > (1 << depth) - 1).any()
        for name, yuv in inputs.items():
            ref = R.yuv420p_to_rgb(yuv, h, w, depth, matrix, full, siting)
            for pad, in_pad in ((16, 0), (4, 2)):                   # (16,24) aligned: the wide form; 2 bytes off: the other
                got = gpu_yuv420p_to_rgb(yuv, h, w, depth, cfg, pad=pad, in_pad=in_pad)
                assert got.dtype == np.float32 and got.shape == ref.shape
                assert got.min() >= 0.0 and got.max() <= 1.0, (depth, cfg, name)
                err = float(np.abs(got.astype(np.float64) - ref).max())
                worst = max(worst, err)
                assert err <= TOL, (depth, cfg, name, pad, in_pad, err)
        assert (gpu_yuv420p_to_rgb(inputs['out_of_gamut'], h, w, depth, cfg)[:, 0] == 1.0).all()
        assert (gpu_yuv420p_to_rgb(inputs['out_of_gamut_mirror'], h, w, depth, cfg)[:, 2] == 1.0).all()
        # a sample above the top code is the top code: bit for bit the same output
        clipped = np.minimum(inputs['above_top'], (1 << depth) - 1).astype(np.uint16)
        assert np.array_equal(gpu_yuv420p_to_rgb(inputs['above_top'], h, w, depth, cfg),
                              gpu_yuv420p_to_rgb(clipped, h, w, depth, cfg))
    print('worst |gpu - fp64| at %dx%d n=%d: %.3g (bound %.3g)' % (h, w, n, worst, TOL))


# ------------------------------------------------------------------ refusals and the ops wrappers
def test_both_entry_points_return_tg_e_arg_without_a_launch():
    from tecogan_pytorch_amd import _lib as L
    lib = L.lib()
    rgb = torch.full((3 * 6 * 6,), 7.0, device=DEV)
    yuv = torch.full((2 * R.frame_samples(6, 6) + 2,), GUARD, dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    out_fn, in_fn = lib.tg_rgb_f32_to_yuv420p16, lib.tg_yuv420p16_to_rgb_f32
    for depth in (8, 9, 11, 14, 16, 0, -10):
        assert out_fn(rgb.data_ptr(), yuv.data_ptr(), 1, 6, 6, depth, 1, 0, 1, st) == E_ARG
        assert b'depth' in lib.tg_last_error_string()
        assert in_fn(yuv.data_ptr(), rgb.data_ptr(), 1, 6, 6, depth, 1, 0, 1, st) == E_ARG
    assert out_fn(rgb.data_ptr(), yuv.data_ptr(), 1, 5, 6, 10, 1, 0, 1, st) == E_ARG           # odd H / W on the way out
    assert out_fn(rgb.data_ptr(), yuv.data_ptr(), 1, 6, 5, 10, 1, 0, 1, st) == E_ARG
    assert b'even' in lib.tg_last_error_string()
    assert out_fn(rgb.data_ptr(), yuv.data_ptr() + 1, 1, 6, 6, 10, 1, 0, 1, st) == E_ARG       # a sample pointer on an odd byte
    assert b'aligned' in lib.tg_last_error_string()
    assert in_fn(yuv.data_ptr() + 1, rgb.data_ptr(), 1, 6, 6, 12, 1, 0, 1, st) == E_ARG
    assert out_fn(None, yuv.data_ptr(), 1, 6, 6, 10, 1, 0, 1, st) == E_ARG
    assert out_fn(rgb.data_ptr(), None, 1, 6, 6, 10, 1, 0, 1, st) == E_ARG
    assert in_fn(None, rgb.data_ptr(), 1, 6, 6, 10, 1, 0, 1, st) == E_ARG
    assert in_fn(yuv.data_ptr(), None, 1, 6, 6, 10, 1, 0, 1, st) == E_ARG
    assert b'null' in lib.tg_last_error_string()
    for m, r, s in ((2, 0, 0), (-1, 0, 0), (0, 2, 0), (0, 0, 2)):
        assert out_fn(rgb.data_ptr(), yuv.data_ptr(), 1, 6, 6, 10, m, r, s, st) == E_ARG
        assert in_fn(yuv.data_ptr(), rgb.data_ptr(), 1, 6, 6, 10, m, r, s, st) == E_ARG
    assert out_fn(rgb.data_ptr(), yuv.data_ptr(), 0, 6, 6, 10, 1, 0, 1, st) == E_ARG
    assert in_fn(yuv.data_ptr(), rgb.data_ptr(), 0, 6, 6, 10, 1, 0, 1, st) == E_ARG
    assert in_fn(yuv.data_ptr(), rgb.data_ptr(), 1, 1, 6, 10, 1, 0, 1, st) == E_ARG
    torch.cuda.synchronize()
    assert bool((yuv == GUARD).all()) and bool((rgb == 7.0).all()), 'a refused call launched'


def test_the_four_420_entry_points_refuse_under_their_own_names_without_a_launch():
    """The four 4:2:0 entry points forward to the launches of the planar ones, which take BT.2020 and depth 8: their own
    checks still come first.  Every refused call is TG_E_ARG, the message names the entry point that was CALLED, and
    nothing is written."""
    from tecogan_pytorch_amd import _lib as L
    lib = L.lib()
    st = torch.cuda.current_stream().cuda_stream
    f32 = torch.full((3 * 6 * 6,), 7.0, device=DEV)                  # fp32 RGB, either direction
    u8 = torch.full((6 * 6 * 3,), GUARD, dtype=torch.uint8, device=DEV)             # uint8 RGB
    yuv = torch.full((2 * R.frame_samples(6, 6) + 2,), GUARD, dtype=torch.uint8, device=DEV)
    y, f, u = yuv.data_ptr(), f32.data_ptr(), u8.data_ptr()
    calls = {      # name -> call(src / dst offset of the samples, n, H, W, depth, matrix); out: the output direction
        'tg_rgb_u8_to_yuv420': (True, None, lambda o, n, H, W, d, m: lib.tg_rgb_u8_to_yuv420(u, y + o, n, H, W, m, 0, 1, st)),
        'tg_yuv420_to_rgb_f32': (False, None, lambda o, n, H, W, d, m: lib.tg_yuv420_to_rgb_f32(y + o, f, n, H, W, m, 0, 1, st)),
        'tg_rgb_f32_to_yuv420p16': (True, 10, lambda o, n, H, W, d, m: lib.tg_rgb_f32_to_yuv420p16(f, y + o, n, H, W, d, m, 0, 1, st)),
        'tg_yuv420p16_to_rgb_f32': (False, 10, lambda o, n, H, W, d, m: lib.tg_yuv420p16_to_rgb_f32(y + o, f, n, H, W, d, m, 0, 1, st)),
    }
    for name, (out, depth, call) in calls.items():
        refused = [(0, 1, 6, 6, depth, 2), (0, 0, 6, 6, depth, 1)]                  # BT.2020; n = 0
        if out:
            refused += [(0, 1, 5, 6, depth, 1), (0, 1, 6, 5, depth, 1)]             # odd H, odd W on the way out
        if depth is not None:
            refused += [(0, 1, 6, 6, 8, 1), (1, 1, 6, 6, depth, 1)]                 # depth 8; a sample pointer on an odd byte
        for args in refused:
            assert call(*args) == E_ARG, (name, args)
            assert lib.tg_last_error_string().startswith(name[3:].encode() + b':'), (name, args, lib.tg_last_error_string())
    torch.cuda.synchronize()
    assert bool((yuv == GUARD).all()) and bool((u8 == GUARD).all()) and bool((f32 == 7.0).all()), 'a refused call launched'


def test_ops_wrappers_equal_the_c_abi_and_refuse_what_the_8_bit_ones_refuse():
    from tecogan_pytorch_amd import _lib as L, ops
    x = _rgb_f32_input(2, 16, 34, seed=1)
    dev = torch.from_numpy(x).to(DEV)
    yuv = _yuv16_inputs(2, 9, 11, 10, seed=1)['above_top']
    ydev = torch.from_numpy(yuv).to(DEV)
    for depth, cfg in ((10, ('bt709', False, 'left')), (12, ('bt601', True, 'center'))):
        got = ops.rgb_f32_to_yuv420p(dev, depth, *cfg)
        assert got.dtype == torch.uint16 and got.shape == (2, R.frame_samples(16, 34))
        assert np.array_equal(got.cpu().numpy(), R.rgb_f32_to_yuv420p(x, depth, *cfg))
        into = torch.zeros_like(got)
        assert ops.rgb_f32_to_yuv420p(dev, depth, *cfg, out=into) is into and torch.equal(into.view(torch.uint8), got.view(torch.uint8))
        back = ops.yuv420p_to_rgb(ydev, 9, 11, depth, *cfg)
        assert back.shape == (2, 3, 9, 11) and np.array_equal(back.cpu().numpy(), gpu_yuv420p_to_rgb(yuv, 9, 11, depth, cfg))
        assert torch.equal(ops.yuv420p_to_rgb(ydev[0], 9, 11, depth, *cfg), back[:1])
        into = torch.zeros_like(back)
        assert ops.yuv420p_to_rgb(ydev, 9, 11, depth, *cfg, out=into) is into and torch.equal(into, back)
    assert np.array_equal(ops.rgb_f32_to_yuv420p(dev, 10).cpu().numpy(), R.rgb_f32_to_yuv420p(x, 10, 'bt709', False, 'left'))
    with pytest.raises(L.TecoganHipError):
        ops.rgb_f32_to_yuv420p(torch.from_numpy(x), 10)              # a CPU tensor
    with pytest.raises(L.TecoganHipError):
        ops.yuv420p_to_rgb(torch.from_numpy(yuv), 9, 11, 10)
    with pytest.raises(L.TecoganHipError):
        ops.yuv420p_to_rgb(ydev, 9, 12, 10)                          # the size does not match
    with pytest.raises(L.TecoganHipError):
        ops.yuv420p_to_rgb(ydev.view(torch.uint8), 9, 11, 10)        # bytes are not samples
    with pytest.raises(L.TecoganHipError):
        ops.rgb_f32_to_yuv420p(dev, 10, out=torch.zeros(2, 5, dtype=torch.uint16, device=DEV))
    with pytest.raises(L.TecoganHipError, match='code -2'):
        ops.rgb_f32_to_yuv420p(dev, 8)
    with pytest.raises(L.TecoganHipError, match='code -2'):
        ops.yuv420p_to_rgb(ydev, 9, 11, 16)
    with pytest.raises(L.TecoganHipError, match='code -2'):
        ops.rgb_f32_to_yuv420p(torch.zeros(1, 3, 5, 6, device=DEV), 10)
    with pytest.raises(L.TecoganHipError, match='code -2'):
        ops.rgb_f32_to_yuv420p(dev, 10, matrix=7)
    with pytest.raises(L.TecoganHipError):
        ops.rgb_f32_to_yuv420p(dev, 10, matrix='bt2020')


# ------------------------------------------------------------------ the stream
def make_net(deg, s):
    from tecogan_pytorch_amd.models.networks import FRNet
    net = FRNet(3, 3, 64, 10, deg, s)
    net.load_state_dict(generator_state_dict(scale=s, degradation=deg), strict=True)
    return net.cuda().eval()


@pytest.fixture(scope='module')
def net4():
    return make_net('BD', 4)


def deep_clip(t, h, w, depth, seed, cfg=('bt709', False, 'left')):
    """(t, frame_bytes) uint8, the bytes of a smooth moving clip at `depth` bits (8: I420 as section 7e has it): the
    float clip converted by the numpy specification at the even size that covers h x w, its Y plane cropped to h x w."""
    he, we = 2 * ((h + 1) // 2), 2 * ((w + 1) // 2)
    clip = smooth_clip(t, 3, he, we, seed=seed)
    if depth == 8:
        u8 = (clip.permute(0, 2, 3, 1) * 255.0).round().clamp(0, 255).to(torch.uint8).numpy()
        full = R8.rgb_to_yuv420(u8, *cfg)
    else:
        full = R.rgb_f32_to_yuv420p(clip.numpy().astype(np.float32), depth, *cfg)
    y, u, v = R.planes(full, he, we)
    out = np.ascontiguousarray(np.concatenate([y[:, :h, :w].reshape(t, -1), u.reshape(t, -1), v.reshape(t, -1)], 1))
    return out.view(np.uint8)


def chunkings(clip):
    """frame by frame (1-D items), and in uneven chunks (2-D items)."""
    t, uneven, pos, sizes = clip.shape[0], [], 0, [2, 5, 1, 11, 3, 7]
    while pos < t:
        m = min(t - pos, sizes[len(uneven) % len(sizes)])
        uneven.append(clip[pos:pos + m])
        pos += m
    return {'frames': [f for f in clip], 'uneven': uneven}


def streamed(net, items, spec, **kw):
    out = [c.copy() for c in net.infer_stream(iter(items), DEV, yuv=spec, **kw)]
    ofb = spec.out_frame_bytes(net.scale)
    assert all(c.dtype == np.uint8 and c.ndim == 2 and c.shape[1] == ofb for c in out)
    return np.concatenate(out, 0) if out else np.zeros((0, ofb), np.uint8)


def lr_frames(clip, spec):
    """The LR frames the stream computes from the clip's bytes: the input op of the spec's depth."""
    from tecogan_pytorch_amd import ops
    cfg = (spec.matrix, spec.full_range, spec.siting)
    if spec.depth == 8:
        return ops.yuv420_to_rgb(torch.from_numpy(clip).to(DEV), spec.h, spec.w, *cfg)
    return ops.yuv420p_to_rgb(torch.from_numpy(clip.view(np.uint16)).to(DEV), spec.h, spec.w, spec.depth, *cfg)


def float_frames(net, lr):
    """The float HR frames of the clip `lr` (t,3,h,w on the device), collected by the test itself: the clip goes
    through enqueue_batch on the test's own ping-pong pair, the way infer_sequence(pipeline=True) drives it, and the
    `after` hook copies the state just written aside.  The uint8 frames of the same run must equal infer_sequence's:
    that ties the float frames to the shipped path."""
    from tecogan_pytorch_amd import _lib as L
    from tecogan_pytorch_amd.models.networks.frnet_infer import clip_batches, enqueue_batch, stream_batch_sizes
    t, c, h, w = lr.shape
    s = net.scale
    lr_ext = torch.cat([torch.zeros(1, c, h, w, device=DEV), lr], 0).contiguous()
    hr = [torch.zeros(1, c, s * h, s * w, device=DEV), torch.empty(1, c, s * h, s * w, device=DEV)]
    u8 = torch.empty(t, s * h, s * w, c, dtype=torch.uint8, device=DEV)
    kept = torch.full((t, c, s * h, s * w), float('nan'), device=DEV)
    with torch.no_grad():
        wk = net._weights_key()
        plan = net._get_plan(1, h, w, DEV, wk=wk)
        main, side = torch.cuda.current_stream(DEV), net._side_stream(DEV)
        side.wait_stream(main)
        batches = clip_batches(t, *stream_batch_sizes())
        ev_f, ev_s = net._events(len(batches))
        zflow = torch.zeros(2 * plan.fh * plan.fw, device=DEV)
        by_addr = {hr[0].data_ptr(): hr[0], hr[1].data_ptr(): hr[1]}
        for b, (i0, cnt) in enumerate(batches):
            def keep(j, addr, i0=i0):
                assert addr == hr[(i0 + j + 1) & 1].data_ptr()
                kept[i0 + j].copy_(by_addr[addr][0])                 # on `main`, directly behind the frame's launch
            enqueue_batch(L.lib(), plan, lambda npair: net._get_plan(npair, h, w, DEV, fnet_only=True, wk=wk), b, i0, cnt,
                          lr_ext.data_ptr() + i0 * c * h * w * 4, c * h * w * 4, (hr[0].data_ptr(), hr[1].data_ptr()),
                          u8.data_ptr() + i0 * s * h * s * w * c, s * h * s * w * c, zflow.data_ptr(),
                          2 * plan.fh * plan.fw * 4, main, side, ev_f[b], ev_s[b - 2] if b >= 2 else None, after=keep)
            ev_s[b].record(main)
        main.wait_stream(side)
    torch.cuda.synchronize()
    plan.check_chain()
    assert not bool(torch.isnan(kept).any())
    assert np.array_equal(u8.cpu().numpy(), net.infer_sequence(lr.cpu(), DEV)), 'the float frames are not the shipped path\'s'
    return kept


def reference(net, clip, spec, cuts=()):
    """ops.rgb_f32_to_yuv420p of the float HR frames, as bytes; a forced cut starts a clip of its own."""
    from tecogan_pytorch_amd import ops
    lr = lr_frames(clip, spec)
    edges = [0] + list(cuts) + [len(clip)]
    hr = torch.cat([float_frames(net, lr[a:b]) for a, b in zip(edges[:-1], edges[1:])], 0)
    out = ops.rgb_f32_to_yuv420p(hr, spec.od, spec.matrix, spec.full_range, spec.siting)
    return out.cpu().numpy().view(np.uint8)


@pytest.mark.parametrize('depth,out_depth', [(8, 10), (10, 10), (12, 12)])
@pytest.mark.parametrize('t', [1, 10])
@pytest.mark.parametrize('h,w,cfg', [(16, 24, ('bt709', False, 'left')), (9, 11, ('bt601', True, 'center'))])
def test_deep_stream_equals_the_op_on_the_float_frames_bit_for_bit(net4, h, w, cfg, t, depth, out_depth):
    from tecogan_pytorch_amd.models.networks import Yuv420, yuv420_planes
    spec = Yuv420(h, w, *cfg, depth=depth, out_depth=out_depth)
    clip = deep_clip(t, h, w, depth, 40 + t, cfg)
    assert clip.shape == (t, spec.frame_bytes)
    ref = reference(net4, clip, spec)
    assert ref.shape == (t, spec.out_frame_bytes(4)) == (t, 2 * (4 * h) * (4 * w) * 3 // 2)
    for name, items in chunkings(clip).items():
        got = streamed(net4, items, spec)
        assert got.shape == ref.shape and np.array_equal(got, ref), (name, int((got != ref).sum()))
    y, u, v = yuv420_planes(got, 4 * h, 4 * w, depth=out_depth)
    assert y.dtype == np.uint16 and y.shape == (t, 4 * h, 4 * w) and u.shape == v.shape == (t, 2 * h, 2 * w)
    assert max(int(y.max()), int(u.max()), int(v.max())) <= (1 << out_depth) - 1
    if depth > 8 and t == 10:                                        # samples in place of bytes: the same stream
        assert np.array_equal(streamed(net4, [clip.view(np.uint16)], spec), ref)


def test_deep_input_with_an_8_bit_output(net4):
    """(12, 8): the new input launch in front of the shipped output path."""
    from tecogan_pytorch_amd import ops
    from tecogan_pytorch_amd.models.networks import Yuv420
    spec = Yuv420(9, 11, depth=12, out_depth=8)
    clip = deep_clip(10, 9, 11, 12, 5)
    hr = net4.infer_sequence(lr_frames(clip, spec).cpu(), DEV)
    ref = ops.rgb_to_yuv420(torch.from_numpy(np.ascontiguousarray(hr)).to(DEV)).cpu().numpy()
    assert np.array_equal(streamed(net4, chunkings(clip)['uneven'], spec), ref)


def test_deep_stream_2x_bi():
    from tecogan_pytorch_amd.models.networks import Yuv420
    net = make_net('BI', 2)
    cfg = ('bt709', True, 'left')
    spec = Yuv420(9, 11, *cfg, depth=10)
    clip = deep_clip(19, 9, 11, 10, 8, cfg)
    ref = reference(net, clip, spec)
    assert ref.shape == (19, 2 * 18 * 22 * 3 // 2)
    assert np.array_equal(streamed(net, chunkings(clip)['uneven'], spec), ref)


def test_deep_stream_with_a_forced_scene_cut(net4):
    from tecogan_pytorch_amd.models.networks import SceneCut, Yuv420
    spec = Yuv420(16, 24, out_depth=10)
    clip = deep_clip(13, 16, 24, 8, 12)
    sc = SceneCut(at=(4,))
    got = streamed(net4, chunkings(clip)['frames'], spec, scene_cut=sc)
    assert sc.cuts == [4]
    assert np.array_equal(got, reference(net4, clip, spec, cuts=(4,)))
    assert not np.array_equal(got[4:], reference(net4, clip, spec)[4:])


def test_resize_with_a_deep_output_is_refused_on_the_device_too(net4):
    from tecogan_pytorch_amd.models.networks import Resize, Yuv420
    with pytest.raises(ValueError, match='8-bit'):
        net4.infer_stream(iter([]), DEV, yuv=Yuv420(16, 24, out_depth=12), resize=Resize(32, 48))
    assert streamed(net4, [], Yuv420(16, 24, out_depth=12)).shape[0] == 0


# ------------------------------------------------------------------ the unchanged path
class _Recorder:
    """Stands around the loaded library: every tg_* entry point that is called is noted by name, then runs."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith('tg_'):
            return fn

        def call(*a):
            self.calls.append(name)
            return fn(*a)
        return call


QUIET = ('tg_last_error_string', 'tg_frnet_plan_flow', 'tg_frnet_plan_chain_status')     # queries, not launches


def _recorded_stream(net, monkeypatch, items, spec):
    from tecogan_pytorch_amd import _lib as L
    rec = _Recorder(L.lib())
    with monkeypatch.context() as mp:
        mp.setattr(L, 'lib', lambda: rec)
        out = streamed(net, items, spec)
    return out, [c for c in rec.calls if c not in QUIET]


def test_default_fields_leave_the_stream_and_its_launches_as_they_were(net4, monkeypatch):
    from tecogan_pytorch_amd import ops
    from tecogan_pytorch_amd.models.networks import Yuv420
    from tecogan_pytorch_amd.models.networks.frnet_infer import clip_batches, stream_batch_sizes
    h, w, t = 16, 24, 21
    clip = deep_clip(t, h, w, 8, 3)
    frames = chunkings(clip)['frames']
    plain, explicit = Yuv420(h, w), Yuv420(h, w, depth=8, out_depth=None)
    streamed(net4, frames, plain)                                   # plans of every batch size exist before recording
    got, kinds = _recorded_stream(net4, monkeypatch, frames, plain)
    got_e, kinds_e = _recorded_stream(net4, monkeypatch, frames, explicit)
    got_8, kinds_8 = _recorded_stream(net4, monkeypatch, frames, Yuv420(h, w, out_depth=8))
    # today's bytes: rgb_to_yuv420 of the RGB frames the stream yields for the same LR input
    lr = ops.yuv420_to_rgb(torch.from_numpy(clip).to(DEV), h, w)
    rgb = np.concatenate([c.copy() for c in net4.infer_stream(iter([lr]), DEV)], 0)
    ref = ops.rgb_to_yuv420(torch.from_numpy(rgb).to(DEV)).cpu().numpy()
    assert np.array_equal(got, ref) and np.array_equal(got_e, ref) and np.array_equal(got_8, ref)
    # the launches, in order, are those of a stream that knows nothing of the new fields
    assert kinds == kinds_e == kinds_8
    assert not [k for k in kinds if 'p16' in k]
    nb = len(clip_batches(t, *stream_batch_sizes()))
    assert kinds.count('tg_frnet_step_srnet') == t and kinds.count('tg_rgb_u8_to_yuv420') == nb
    assert kinds.count('tg_yuv420_to_rgb_f32') == nb and kinds.count('tg_frnet_step_phase') == nb
    # and the deep output adds ONE launch behind every frame, drops the per-batch one, and moves nothing else
    _, kinds_10 = _recorded_stream(net4, monkeypatch, frames, Yuv420(h, w, out_depth=10))
    assert kinds_10.count('tg_rgb_f32_to_yuv420p16') == t and 'tg_rgb_u8_to_yuv420' not in kinds_10
    at = [k for k, name in enumerate(kinds_10) if name == 'tg_rgb_f32_to_yuv420p16']
    assert all(kinds_10[k - 1] == 'tg_frnet_step_srnet' for k in at)
    assert [k for k in kinds_10 if k != 'tg_rgb_f32_to_yuv420p16'] == [k for k in kinds if k != 'tg_rgb_u8_to_yuv420']


# ------------------------------------------------------------------ the model wrapper and the CLI
def test_cli_y4m_p10_in_y4m_p10_out(tmp_path):
    import yaml
    from tecogan_pytorch_amd import main as M
    from tecogan_pytorch_amd.data.y4m import Y4MReader
    from tecogan_pytorch_amd.models.networks import Yuv420
    pth = str(tmp_path / 'G_iter7.pth')
    torch.save(generator_state_dict(scale=4, degradation='BD'), pth)
    opt = M.default_opt()
    opt['model']['generator']['load_path'] = pth
    yml = str(tmp_path / 'infer.yml')
    with open(yml, 'w') as f:
        yaml.safe_dump(opt, f)
    h, w, t = 16, 24, 12
    cfg = ('bt601', True, 'center')
    clip = deep_clip(t, h, w, 10, 31, cfg)
    src, dst, dst8 = str(tmp_path / 'in.y4m'), str(tmp_path / 'out.y4m'), str(tmp_path / 'out8.y4m')
    with open(src, 'wb') as f:
        f.write(b'YUV4MPEG2 W24 H16 F25:1 Ip A1:1 C420p10 XYSCSS=420P10 XCOLORRANGE=FULL\n')
        for fr in clip:
            f.write(b'FRAME\n' + fr.tobytes())
    M.main(['--mode', 'infer', '--opt', yml, '--input', src, '--output', dst, '--yuv-matrix', 'bt601', '--yuv-siting', 'center'])
    rd = Y4MReader(io.BytesIO(open(dst, 'rb').read()), depths=(8, 10, 12))
    assert (rd.w, rd.h, rd.depth, rd.siting, rd.full_range) == (96, 64, 10, None, True)
    assert rd.header['tags'] == ['F25:1', 'A1:1', 'C420p10', 'XYSCSS=420P10', 'XCOLORRANGE=FULL']
    got = np.stack([fr.copy() for fr in rd])
    # the model wrapper pads the front of the longer items as it pads 8-bit ones; the engine on the padded clip is the reference
    n_pad = opt['test']['num_pad_front']
    assert opt['test'].get('padding_mode', 'reflect') == 'reflect' and 0 < n_pad < t
    net = make_net('BD', 4)
    spec = Yuv420(h, w, *cfg, depth=10)
    padded = np.concatenate([clip[1:1 + n_pad][::-1], clip], 0)
    ref = streamed(net, [padded], spec)[n_pad:]
    assert got.shape == ref.shape == (t, spec.out_frame_bytes(4)) and np.array_equal(got, ref)
    # --output-depth 8 after a 10-bit input: an 8-bit header with the siting's tags, frames of half the bytes
    M.main(['--mode', 'infer', '--opt', yml, '--input', src, '--output', dst8, '--yuv-matrix', 'bt601', '--yuv-siting', 'center',
            '--output-depth', '8'])
    rd8 = Y4MReader(io.BytesIO(open(dst8, 'rb').read()))
    assert (rd8.w, rd8.h, rd8.siting, rd8.full_range) == (96, 64, 'center', True)
    assert rd8.header['tags'] == ['F25:1', 'A1:1', 'C420jpeg', 'XYSCSS=420JPEG', 'XCOLORRANGE=FULL']
    got8 = np.stack([fr.copy() for fr in rd8])
    ref8 = streamed(net, [padded], Yuv420(h, w, *cfg, depth=10, out_depth=8))[n_pad:]
    assert got8.shape == (t, 64 * 96 * 3 // 2) and np.array_equal(got8, ref8)
