"""Semi-planar YUV on the GPU: NV12 / NV16 / NV24 and P010 ... P412 through the three entry
points of the C ABI, with guard bytes around every output, against tests/semiplanar_ref.py.

The contract is a reduction to the planar one.  Out: the bytes and words equal to_semi of what tests/yuv_planar_ref.py
specifies for the same RGB.  In: the floats equal, bit for bit, those of tg_yuv_planar_to_rgb_f32 on to_planar(frame),
and so lie within the bound against fp64 derived per matrix in tests/test_hip_yuv_planar.py (TOL, imported).  Then the
wrappers of tecogan_pytorch_amd.semiplanar, FRNet.infer_stream(yuv=Yuv(..., layout='semi')) and the command line, each
against the planar run on the relaid frames."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from procedural_weights import generator_state_dict
from tests import ops_cases as OC
from tests import semiplanar_ref as S
from tests import yuv_planar_ref as P
from tests.test_hip_ops_boundary import bad_versions
from tests.test_hip_yuv_depth import QUIET, _Recorder, chunkings, make_net
from tests.test_hip_yuv_planar import (ALL_CFGS, E_ARG, GUARD, ONE_CFG, TOL, _codes, _guarded, _guards_intact, _placed,
                                       _rgb_f32_inputs, _rgb_u8_inputs, _stream, gpu_yuv_to_rgb, planar_clip, streamed)

DEV = torch.device('cuda', 0)
ROOT_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT_SHAPES = {'444': [(2, 2), (3, 5), (4, 8), (18, 22)], '422': [(2, 2), (3, 6), (5, 10), (4, 8), (64, 130)],
              '420': [(2, 2), (4, 6), (6, 8), (18, 22), (16, 24)]}
OUT_CASES = [(c, H, W) for c in P.CHROMAS for (H, W) in OUT_SHAPES[c]]
NEW = ('tg_yuv_semiplanar_to_rgb_f32', 'tg_rgb_u8_to_yuv_semiplanar', 'tg_rgb_f32_to_yuv_semiplanar16')
PLANAR = ('tg_yuv_planar_to_rgb_f32', 'tg_rgb_u8_to_yuv_planar', 'tg_rgb_f32_to_yuv_planar16')


def gpu_rgb_u8_to_semi(rgb, chroma, cfg, pad=16, in_pad=0):
    """tg_rgb_u8_to_yuv_semiplanar through the C ABI on (n,H,W,3) uint8 numpy -> (n, frame_bytes) uint8 numpy."""
    from tecogan_pytorch_amd import _lib as L
    n, H, W, _ = rgb.shape
    hold, src = _placed(rgb, in_pad)
    buf, out = _guarded(n * P.frame_bytes(H, W, chroma), pad, torch.uint8)
    c, m, r, s = _codes(chroma, *cfg)
    L.check(L.lib().tg_rgb_u8_to_yuv_semiplanar(src, out.data_ptr(), n, H, W, c, m, r, s, _stream()), NEW[1])
    torch.cuda.synchronize()
    assert _guards_intact(buf, pad), 'tg_rgb_u8_to_yuv_semiplanar wrote outside its output'
    return out.cpu().numpy().reshape(n, -1)


def gpu_rgb_f32_to_semi(rgb, chroma, depth, cfg, pad=16, in_pad=0):
    """tg_rgb_f32_to_yuv_semiplanar16 through the C ABI on (n,3,H,W) float32 numpy -> (n, frame_samples) uint16 numpy."""
    from tecogan_pytorch_amd import _lib as L
    n, _, H, W = rgb.shape
    hold, src = _placed(rgb, in_pad)
    buf, out = _guarded(n * P.frame_bytes(H, W, chroma, depth), pad, torch.uint16)
    c, m, r, s = _codes(chroma, *cfg)
    L.check(L.lib().tg_rgb_f32_to_yuv_semiplanar16(src, out.data_ptr(), n, H, W, c, depth, m, r, s, _stream()), NEW[2])
    torch.cuda.synchronize()
    assert _guards_intact(buf, pad), 'tg_rgb_f32_to_yuv_semiplanar16 wrote outside its output'
    return out.cpu().numpy().reshape(n, -1)


def gpu_semi_to_rgb(yuv, h, w, chroma, depth, cfg, pad=16, in_pad=0):
    """tg_yuv_semiplanar_to_rgb_f32 through the C ABI on (n, frame_samples) uint8 / uint16 numpy -> (n,3,h,w) float32."""
    from tecogan_pytorch_amd import _lib as L
    n = yuv.shape[0]
    assert yuv.dtype == (np.uint8 if depth == 8 else np.uint16) and yuv.shape[1] == P.frame_samples(h, w, chroma)
    hold, src = _placed(yuv, in_pad)
    buf, out = _guarded(n * 3 * h * w * 4, pad, torch.float32)
    c, m, r, s = _codes(chroma, *cfg)
    L.check(L.lib().tg_yuv_semiplanar_to_rgb_f32(src, out.data_ptr(), n, h, w, c, depth, m, r, s, _stream()), NEW[0])
    torch.cuda.synchronize()
    assert _guards_intact(buf, pad), 'tg_yuv_semiplanar_to_rgb_f32 wrote outside its output'      # (16 bytes either side)
    return out.cpu().numpy().reshape(n, 3, h, w)


# ------------------------------------------------------------------ the two output directions: identity
def _cfgs_of(chroma, H, W):
    """All sitings, matrices and ranges at the small shapes (up to 64 pixels: they include the wide form, W = 2 mod 4
    and odd sizes), one configuration at the large ones."""
    return ALL_CFGS if H * W <= 64 else [ONE_CFG[chroma]]


def _u8_inputs(n, H, W, seed):
    return dict(_rgb_u8_inputs(n, H, W, seed), zeros=np.zeros((n, H, W, 3), np.uint8),
                ones=np.full((n, H, W, 3), 255, np.uint8))


def _f32_inputs(n, H, W, seed):
    x = _rgb_f32_inputs(n, H, W, seed)                              # 'random': below 0, above 1, NaN, infinities, ties
    assert (x['random'] < 0).any() and (x['random'] > 1).any()
    return dict(x, zeros=np.zeros((n, 3, H, W), np.float32), ones=np.ones((n, 3, H, W), np.float32))


@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('chroma,H,W', OUT_CASES)
def test_rgb_u8_to_semi_equals_the_specification_byte_for_byte(chroma, H, W, n):
    inputs = _u8_inputs(n, H, W, seed=H * 1000 + W + n)
    for cfg in _cfgs_of(chroma, H, W):
        for name, rgb in inputs.items():
            ref = S.rgb_u8_to_semi(rgb, chroma, *cfg)
            got = gpu_rgb_u8_to_semi(rgb, chroma, cfg)
            assert got.shape == ref.shape and got.dtype == ref.dtype
            assert np.array_equal(got, ref), (cfg, name, int((got != ref).sum()), np.flatnonzero(got[0] != ref[0])[:8])


@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('chroma,H,W', OUT_CASES)
def test_rgb_f32_to_semi_equals_the_specification_word_for_word(chroma, H, W, n):
    inputs = _f32_inputs(n, H, W, seed=H * 1000 + W + n)
    for depth in (10, 12):
        for cfg in _cfgs_of(chroma, H, W):
            for name, rgb in inputs.items():
                ref = S.rgb_f32_to_semi(rgb, chroma, depth, *cfg)
                got = gpu_rgb_f32_to_semi(rgb, chroma, depth, cfg)
                assert got.shape == ref.shape and got.dtype == ref.dtype
                assert np.array_equal(got, ref), (depth, cfg, name, int((got != ref).sum()))
                assert not (got & ((1 << (16 - depth)) - 1)).any()  # the low bits are zero


@pytest.mark.parametrize('chroma', P.CHROMAS)
def test_all_three_over_more_than_one_workgroup(chroma):
    """n = 2 at 36x40: 720 strips on the way in, 720 (360 at 4:2:0) on the way out -- more than one block of 256
    threads, the last one partly idle."""
    n, H, W = 2, 36, 40
    for siting in P.SITINGS:
        cfg = ('bt2020', siting == 'left', siting)
        rgb = _rgb_u8_inputs(n, H, W, seed=7)['random']
        assert np.array_equal(gpu_rgb_u8_to_semi(rgb, chroma, cfg), S.rgb_u8_to_semi(rgb, chroma, *cfg))
        x = _rgb_f32_inputs(n, H, W, seed=8)['random']
        assert np.array_equal(gpu_rgb_f32_to_semi(x, chroma, 10, cfg), S.rgb_f32_to_semi(x, chroma, 10, *cfg))
        for depth in (8, 12):
            semi = _semi_inputs(n, H, W, chroma, depth, 9)['random']
            got = gpu_semi_to_rgb(semi, H, W, chroma, depth, cfg)
            assert np.array_equal(got, gpu_yuv_to_rgb(S.to_planar(semi, H, W, chroma, depth), H, W, chroma, depth, cfg))


@pytest.mark.parametrize('chroma', P.CHROMAS)
def test_a_base_one_sample_off_its_wide_alignment_takes_the_element_wide_form(chroma):
    """W % 4 == 0 and, once per function, the output or the input one sample off: the same bytes, guards intact."""
    n, H, W = 2, 6, 8
    cfg = ('bt709', False, 'left')
    rgb = _rgb_u8_inputs(n, H, W, seed=3)['random']
    ref = S.rgb_u8_to_semi(rgb, chroma, *cfg)
    assert np.array_equal(gpu_rgb_u8_to_semi(rgb, chroma, cfg), ref)                   # the wide form
    assert np.array_equal(gpu_rgb_u8_to_semi(rgb, chroma, cfg, pad=17), ref)           # the output one byte off a dword
    assert np.array_equal(gpu_rgb_u8_to_semi(rgb, chroma, cfg, in_pad=1), ref)         # the input
    x = _rgb_f32_inputs(n, H, W, seed=4)['random']
    ref = S.rgb_f32_to_semi(x, chroma, 12, *cfg)
    assert np.array_equal(gpu_rgb_f32_to_semi(x, chroma, 12, cfg), ref)
    assert np.array_equal(gpu_rgb_f32_to_semi(x, chroma, 12, cfg, pad=18), ref)        # the output one sample off 8 bytes
    assert np.array_equal(gpu_rgb_f32_to_semi(x, chroma, 12, cfg, in_pad=4), ref)      # the input one float off 16 bytes
    for depth, one in ((8, 1), (10, 2)):
        semi = _semi_inputs(n, H, W, chroma, depth, 5)['random']
        wide = gpu_semi_to_rgb(semi, H, W, chroma, depth, cfg)
        assert np.array_equal(wide, gpu_yuv_to_rgb(S.to_planar(semi, H, W, chroma, depth), H, W, chroma, depth, cfg))
        assert np.array_equal(gpu_semi_to_rgb(semi, H, W, chroma, depth, cfg, in_pad=one), wide)   # the input one sample off
        assert np.array_equal(gpu_semi_to_rgb(semi, H, W, chroma, depth, cfg, pad=20), wide)       # the output one float off


# ------------------------------------------------------------------ the input direction
def _semi_inputs(n, h, w, chroma, depth, seed):
    """Semi-planar frames: random codes, the out-of-gamut and below-black constants; above 8 bits every word carries
    random low bits."""
    rng = np.random.default_rng(seed)
    ns, top = P.frame_samples(h, w, chroma), (1 << depth) - 1
    dt = np.uint8 if depth == 8 else np.uint16
    ch, cw = P.chroma_size(h, w, chroma)

    def const(y, u, v):
        one = np.concatenate([np.full(h * w, y), np.full(ch * cw, u), np.full(ch * cw, v)]).astype(dt)
        return np.broadcast_to(one, (n, ns)).copy()
    planar = {'random': rng.integers(0, top + 1, (n, ns)).astype(dt), 'out_of_gamut': const(top, 0, top),
              'below_black': const(0, top, 0)}
    out = {}
    for name, x in planar.items():
        semi = S.to_semi(x, h, w, chroma, depth)
        if depth > 8:
            low = rng.integers(0, 1 << (16 - depth), semi.shape).astype(np.uint16)
            low[:, 0] = low[:, -1] = (1 << (16 - depth)) - 1          # (a luma and a chroma word at the least)
            semi = semi | low
            assert np.array_equal(S.to_planar(semi, h, w, chroma, depth), x)
        out[name] = semi
    return out


@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('depth', P.DEPTHS)
@pytest.mark.parametrize('h,w', [(2, 2), (3, 5), (9, 11), (16, 24)])
def test_semi_to_rgb_equals_the_planar_entry_point_bit_for_bit_and_is_within_the_bound_of_fp64(h, w, depth, n):
    worst = dict.fromkeys(TOL, 0.0)
    for chroma in P.CHROMAS:
        inputs = _semi_inputs(n, h, w, chroma, depth, seed=h * 1000 + w + n + depth)
        for cfg in ALL_CFGS:
            for name, semi in inputs.items():
                got = gpu_semi_to_rgb(semi, h, w, chroma, depth, cfg)               # (16,24) aligned: the wide form
                twin = gpu_yuv_to_rgb(S.to_planar(semi, h, w, chroma, depth), h, w, chroma, depth, cfg)
                assert got.dtype == np.float32 and got.shape == twin.shape == (n, 3, h, w)
                assert np.array_equal(got.view(np.uint32), twin.view(np.uint32)), (chroma, cfg, name)
                assert got.min() >= 0.0 and got.max() <= 1.0, (chroma, cfg, name)
                err = float(np.abs(got.astype(np.float64) - S.semi_to_rgb(semi, h, w, chroma, depth, *cfg)).max())
                worst[cfg[0]] = max(worst[cfg[0]], err)
                assert err <= TOL[cfg[0]], (chroma, cfg, name, err)
    print('worst |gpu - fp64| at %dx%d n=%d depth %d: %s (bounds %s)'
          % (h, w, n, depth, {k: '%.3g' % v for k, v in worst.items()}, TOL))


# ------------------------------------------------------------------ refusals
def test_entry_points_return_tg_e_arg_without_a_launch():
    from tecogan_pytorch_amd import _lib as L
    lib = L.lib()
    rgb = torch.full((3 * 6 * 6,), 7.0, device=DEV)
    u8 = torch.full((3 * 6 * 6 + 4,), 9, dtype=torch.uint8, device=DEV)
    yuv = torch.full((2 * P.frame_samples(6, 6, '444') + 8,), GUARD, dtype=torch.uint8, device=DEV)
    st = _stream()
    fin, out8, out16 = lib.tg_yuv_semiplanar_to_rgb_f32, lib.tg_rgb_u8_to_yuv_semiplanar, lib.tg_rgb_f32_to_yuv_semiplanar16
    R, U, Y = rgb.data_ptr(), u8.data_ptr(), yuv.data_ptr()
    for chroma in (3, -1, 420):
        assert fin(Y, R, 1, 6, 6, chroma, 8, 1, 0, 1, st) == E_ARG
        assert b'chroma' in lib.tg_last_error_string() and b'semiplanar' in lib.tg_last_error_string()
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
    assert fin(Y + 1, R, 1, 6, 6, 2, 10, 1, 0, 1, st) == E_ARG                                  # 16-bit words on an odd byte
    assert b'aligned' in lib.tg_last_error_string()
    assert fin(Y, R + 2, 1, 6, 6, 2, 8, 1, 0, 1, st) == E_ARG                                   # an fp32 pointer off a float
    assert out16(R, Y + 1, 1, 6, 6, 2, 10, 1, 0, 1, st) == E_ARG and out16(R + 1, Y, 1, 6, 6, 2, 10, 1, 0, 1, st) == E_ARG
    torch.cuda.synchronize()
    assert bool((yuv == GUARD).all()) and bool((rgb == 7.0).all()) and bool((u8 == 9).all()), 'a refused call launched'


# ------------------------------------------------------------------ the wrappers
def test_wrappers_equal_the_c_abi_and_refuse_bad_arguments():
    from tecogan_pytorch_amd import _lib as L, ops, semiplanar
    rgb = _rgb_u8_inputs(2, 5, 10, seed=1)['random']
    x = _rgb_f32_inputs(2, 5, 10, seed=2)['random']
    dev8, devf = torch.from_numpy(rgb).to(DEV), torch.from_numpy(x).to(DEV)
    for chroma, cfg in (('422', ('bt2020', False, 'left')), ('444', ('bt601', True, 'center'))):
        got = semiplanar.from_rgb(dev8, chroma, *cfg)
        assert got.dtype == torch.uint8 and got.shape == (2, ops.yuv_frame_samples(5, 10, chroma))
        assert np.array_equal(got.cpu().numpy(), gpu_rgb_u8_to_semi(rgb, chroma, cfg))
        assert np.array_equal(semiplanar.to_planar(got.cpu().numpy(), 5, 10, chroma, 8), ops.rgb_to_yuv(dev8, chroma, *cfg).cpu().numpy())
        deep = semiplanar.from_rgb_f32(devf, chroma, 12, *cfg)
        assert deep.dtype == torch.uint16 and np.array_equal(deep.cpu().numpy(), gpu_rgb_f32_to_semi(x, chroma, 12, cfg))
        into = torch.zeros_like(deep)
        assert semiplanar.from_rgb_f32(devf, chroma, 12, *cfg, out=into) is into
        assert torch.equal(into.view(torch.uint8), deep.view(torch.uint8))
        back = semiplanar.to_rgb(got, 5, 10, chroma, 8, *cfg)
        assert back.shape == (2, 3, 5, 10) and np.array_equal(back.cpu().numpy(), gpu_semi_to_rgb(got.cpu().numpy(), 5, 10, chroma, 8, cfg))
        assert torch.equal(semiplanar.to_rgb(got[0], 5, 10, chroma, 8, *cfg), back[:1])
        back12 = semiplanar.to_rgb(deep, 5, 10, chroma, 12, *cfg)
        assert np.array_equal(back12.cpu().numpy(), gpu_semi_to_rgb(deep.cpu().numpy(), 5, 10, chroma, 12, cfg))
        into = torch.zeros_like(back12)
        assert semiplanar.to_rgb(deep, 5, 10, chroma, 12, *cfg, out=into) is into and torch.equal(into, back12)
    for bad in (lambda: semiplanar.from_rgb(torch.from_numpy(rgb)), lambda: semiplanar.from_rgb(dev8, '411'),
                lambda: semiplanar.from_rgb(dev8, '444', matrix='bt2100'),
                lambda: semiplanar.to_rgb(dev8.view(2, -1), 5, 10, '420'),
                lambda: semiplanar.to_rgb(semiplanar.from_rgb(dev8, '444'), 5, 10, '444', 10),       # bytes are not words
                lambda: semiplanar.from_rgb_f32(devf, '444', 10, out=torch.zeros(2, 5, dtype=torch.uint16, device=DEV))):
        with pytest.raises(L.TecoganHipError):
            bad()
    with pytest.raises(L.TecoganHipError, match='code -2'):
        semiplanar.from_rgb(dev8[:, :, :9].contiguous(), '422')     # an odd width
    with pytest.raises(L.TecoganHipError, match='code -2'):
        semiplanar.from_rgb_f32(devf, '444', 8)


def _wrapper_rows(semiplanar):
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8, device=DEV)
    u16 = lambda *s: torch.zeros(*s, dtype=torch.uint16, device=DEV)
    f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=DEV)
    ns = P.frame_samples(6, 8, '420')
    return [
        ('to_rgb 8', semiplanar.to_rgb, dict(yuv=u8(2, ns), h=6, w=8, out=f32(2, 3, 6, 8)), NEW[0]),
        ('to_rgb 10', semiplanar.to_rgb, dict(yuv=u16(2, ns), h=6, w=8, depth=10, out=f32(2, 3, 6, 8)), NEW[0]),
        ('from_rgb', semiplanar.from_rgb, dict(rgb_hwc=u8(2, 6, 8, 3)), NEW[1]),
        ('from_rgb_f32', semiplanar.from_rgb_f32, dict(rgb_chw=f32(2, 3, 6, 8), depth=12, out=u16(2, ns)), NEW[2]),
    ]


def test_every_tensor_operand_of_the_wrappers_is_checked_before_the_library(monkeypatch):
    """The boundary rule of ops (tests/test_hip_ops_boundary.py), applied to the wrappers that live outside ops.py: the
    valid call reaches exactly its entry point, and with any one tensor operand replaced by a CPU copy, another dtype or
    a non-dense tensor of the same shape it is refused before anything reaches the library."""
    from tecogan_pytorch_amd import ops, semiplanar
    from tecogan_pytorch_amd._lib import TecoganHipError
    seen = OC.recorder(monkeypatch, ops)
    for label, fn, kwargs, entry in _wrapper_rows(semiplanar):
        del seen[:]
        fn(**kwargs)
        assert seen == [entry], (label, seen)
        operands = list(OC.tensor_paths(kwargs))
        assert len(operands) >= 1, label
        for path, t in operands:
            for what, bad in bad_versions(t, False):
                del seen[:]
                with pytest.raises(TecoganHipError):
                    fn(**OC.replaced(kwargs, path, bad))
                assert seen == [], f'{label}: {what} tensor for {path}: {seen} was reached before the refusal'


# ------------------------------------------------------------------ the stream
@pytest.fixture(scope='module')
def net4():
    return make_net('BD', 4)


def _sides(spec):
    """(input relayout, output relayout) of a spec: identity for a planar side."""
    def relay(fn, h, w, chroma, depth, on):
        def go(frames):                                             # (t, frame_bytes) uint8 -> the same, relaid
            if not on:
                return frames
            x = frames if depth == 8 else np.ascontiguousarray(frames).view(np.uint16)
            return np.ascontiguousarray(fn(x, h, w, chroma, depth)).view(np.uint8)
        return go
    return relay, spec.layout == 'semi', spec.ol == 'semi'


def run_both(net, planar_in, spec, items_of=lambda clip: [clip], H=None, W=None, **kw):
    """The stream of `spec` on the semi-planar form of the planar clip, and what it must yield: the relaid bytes of the
    same stream run with the planar layout on the planar clip.  kw are built per run (a SceneCut serves one stream)."""
    from tecogan_pytorch_amd.models.networks import Yuv
    import dataclasses
    relay, semi_in, semi_out = _sides(spec)
    H, W = (net.scale * spec.h, net.scale * spec.w) if H is None else (H, W)
    clip = relay(S.to_semi, spec.h, spec.w, spec.chroma, spec.depth, semi_in)(planar_in)
    if semi_in:
        assert np.array_equal(relay(S.to_planar, spec.h, spec.w, spec.chroma, spec.depth, True)(clip), planar_in)
    ofb = spec.out_size_bytes(H, W)
    got = streamed(net, items_of(clip), spec, ofb=ofb, **{k: v() for k, v in kw.items()})
    twin = dataclasses.replace(spec, layout='planar', out_layout='planar')
    assert isinstance(twin, Yuv) and twin.input_launch()[0] == PLANAR[0]
    ref = streamed(net, items_of(planar_in), twin, ofb=ofb, **{k: v() for k, v in kw.items()})
    return got, relay(S.to_semi, H, W, spec.oc, spec.od, semi_out)(ref)


CONVERSIONS = {                        # chroma, out_chroma, depth, out_depth, layout, out_layout, (matrix, full, siting)
    'nv12_to_nv12': ('420', None, 8, None, 'semi', None, ('bt709', False, 'left')),
    'p010_to_p010': ('420', None, 10, None, 'semi', None, ('bt2020', False, 'left')),
    'nv12_to_444p': ('420', '444', 8, None, 'semi', 'planar', ('bt601', True, 'center')),
    '422p10_to_p210': ('422', None, 10, None, 'planar', 'semi', ('bt2020', True, 'left')),
    'nv24_to_nv12': ('444', '420', 8, None, 'semi', None, ('bt709', False, 'center')),
}


@pytest.mark.parametrize('t', [1, 10])
@pytest.mark.parametrize('h,w', [(16, 24), (9, 11)])
@pytest.mark.parametrize('conv', sorted(CONVERSIONS))
def test_stream_equals_the_planar_stream_relaid_bit_for_bit(net4, conv, h, w, t):
    from tecogan_pytorch_amd.models.networks import Yuv, yuv_semiplanes
    chroma, oc, depth, od, layout, ol, cfg = CONVERSIONS[conv]
    spec = Yuv(h, w, chroma, oc, *cfg, depth=depth, out_depth=od, layout=layout, out_layout=ol)
    planar_in = planar_clip(t, h, w, chroma, depth, 40 + t, cfg)
    assert planar_in.shape == (t, spec.frame_bytes)
    for name in ('frames', 'uneven'):
        got, ref = run_both(net4, planar_in, spec, items_of=lambda clip: chunkings(clip)[name])
        assert got.shape == ref.shape == (t, spec.out_frame_bytes(4)) and np.array_equal(got, ref), (name, int((got != ref).sum()))
    if spec.ol == 'semi':
        ch, cw = P.chroma_size(4 * h, 4 * w, spec.oc)
        y, uv = yuv_semiplanes(got, 4 * h, 4 * w, spec.oc, spec.od)
        assert y.shape == (t, 4 * h, 4 * w) and uv.shape == (t, ch, cw, 2)
        if spec.od > 8:
            assert not (y & ((1 << (16 - spec.od)) - 1)).any() and not (uv & ((1 << (16 - spec.od)) - 1)).any()


def test_stream_with_a_forced_scene_cut(net4):
    from tecogan_pytorch_amd.models.networks import SceneCut, Yuv
    cfg = ('bt2020', False, 'left')
    spec = Yuv(16, 24, '420', None, *cfg, depth=10, layout='semi')
    planar_in = planar_clip(13, 16, 24, '420', 10, 12, cfg)
    cuts = []

    def cut():
        cuts.append(SceneCut(at=(4,)))
        return cuts[-1]
    got, ref = run_both(net4, planar_in, spec, items_of=lambda clip: chunkings(clip)['frames'], scene_cut=cut)
    assert [c.cuts for c in cuts] == [[4], [4]]
    assert np.array_equal(got, ref)
    plain, _ = run_both(net4, planar_in, spec)
    assert np.array_equal(got[:4], plain[:4]) and not np.array_equal(got[4:], plain[4:])


def test_stream_with_a_resize_on_an_8_bit_semi_planar_output(net4):
    from tecogan_pytorch_amd.models.networks import Resize, Yuv
    cfg = ('bt709', False, 'center')
    spec = Yuv(9, 11, '420', '422', *cfg, layout='semi')            # nv12 in, nv16 out at an odd height
    planar_in = planar_clip(10, 9, 11, '420', 8, 6, cfg)
    got, ref = run_both(net4, planar_in, spec, items_of=lambda clip: chunkings(clip)['uneven'], H=45, W=70,
                        resize=lambda: Resize(45, 70))
    assert got.shape == (10, P.frame_bytes(45, 70, '422')) and np.array_equal(got, ref)
    with pytest.raises(ValueError, match='even width'):
        net4.infer_stream(iter([]), DEV, yuv=spec, resize=Resize(45, 71))


def test_stream_2x_bi():
    from tecogan_pytorch_amd.models.networks import Yuv
    net = make_net('BI', 2)
    cfg = ('bt2020', True, 'left')
    spec = Yuv(9, 11, '444', '422', *cfg, depth=12, out_depth=10, layout='semi')     # p412 in, p210 out
    planar_in = planar_clip(19, 9, 11, '444', 12, 8, cfg)
    got, ref = run_both(net, planar_in, spec, items_of=lambda clip: chunkings(clip)['uneven'])
    assert got.shape == (19, 2 * 2 * 18 * 22) and np.array_equal(got, ref)


def test_deinterlace_with_a_semi_planar_input_is_refused_before_any_item_is_pulled(net4):
    from tecogan_pytorch_amd.models.networks import Deinterlace, Yuv
    pulled = []

    def items():
        pulled.append(1)
        yield np.zeros(Yuv(16, 24).frame_bytes, np.uint8)
    with pytest.raises(ValueError, match='semi-planar'):
        net4.infer_stream(items(), DEV, yuv=Yuv(16, 24, layout='semi'), deinterlace=Deinterlace())
    assert pulled == []


# ------------------------------------------------------------------ which entry points a stream calls
def _recorded_stream(net, monkeypatch, items, spec):
    from tecogan_pytorch_amd import _lib as L
    rec = _Recorder(L.lib())
    with monkeypatch.context() as mp:
        mp.setattr(L, 'lib', lambda: rec)
        out = streamed(net, items, spec)
    return out, [c for c in rec.calls if c not in QUIET]


def test_planar_streams_call_none_of_the_new_entry_points_and_a_semi_planar_side_none_of_the_planar_ones(net4, monkeypatch):
    from tecogan_pytorch_amd.models.networks import Yuv, Yuv420
    h, w, t = 16, 24, 11
    cfg = ('bt709', False, 'left')
    clip = planar_clip(t, h, w, '420', 8, 3, cfg)
    frames = chunkings(clip)['frames']
    streamed(net4, frames, Yuv420(h, w))                            # plans of every batch size exist before recording
    _, k420 = _recorded_stream(net4, monkeypatch, frames, Yuv420(h, w))
    _, k420_10 = _recorded_stream(net4, monkeypatch, frames, Yuv420(h, w, out_depth=10))
    _, kp = _recorded_stream(net4, monkeypatch, frames, Yuv(h, w))
    _, kp_10 = _recorded_stream(net4, monkeypatch, frames, Yuv(h, w, out_depth=10))
    assert not [k for k in k420 + k420_10 + kp + kp_10 if k in NEW]
    assert PLANAR[0] in kp and PLANAR[1] in kp and PLANAR[2] in kp_10
    new_of = dict(zip(PLANAR, NEW))
    semi = S.to_semi(clip, h, w, '420', 8)
    _, ks = _recorded_stream(net4, monkeypatch, [f for f in semi], Yuv(h, w, layout='semi'))
    assert not [k for k in ks if k in PLANAR] and ks == [new_of.get(k, k) for k in kp]          # one for one, in place
    _, ks_10 = _recorded_stream(net4, monkeypatch, [f for f in semi], Yuv(h, w, out_depth=10, layout='semi'))
    assert not [k for k in ks_10 if k in PLANAR] and ks_10 == [new_of.get(k, k) for k in kp_10]
    _, k_in = _recorded_stream(net4, monkeypatch, [f for f in semi], Yuv(h, w, layout='semi', out_layout='planar'))
    assert NEW[0] in k_in and PLANAR[0] not in k_in and PLANAR[1] in k_in and NEW[1] not in k_in
    _, k_out = _recorded_stream(net4, monkeypatch, frames, Yuv(h, w, out_layout='semi'))
    assert PLANAR[0] in k_out and NEW[0] not in k_out and NEW[1] in k_out and PLANAR[1] not in k_out


# ------------------------------------------------------------------ the CLI
def _cli(args, timeout=240, **kw):
    """python -m tecogan_pytorch_amd.main in a fresh child process with its own time limit."""
    env = dict(os.environ, PYTHONPATH=ROOT_DIR + os.pathsep + os.environ.get('PYTHONPATH', ''))
    r = subprocess.run([sys.executable, '-m', 'tecogan_pytorch_amd.main', '--mode', 'infer', *args], cwd=ROOT_DIR, env=env,
                       capture_output=True, timeout=timeout, **kw)
    assert r.returncode == 0, r.stderr[-3000:]
    return r


def _yml(tmp_path):
    import yaml
    from tecogan_pytorch_amd import main as M
    pth = str(tmp_path / 'G_iter7.pth')
    torch.save(generator_state_dict(scale=4, degradation='BD'), pth)
    opt = M.default_opt()
    opt['model']['generator']['load_path'] = pth
    yml = str(tmp_path / 'infer.yml')
    with open(yml, 'w') as f:
        yaml.safe_dump(opt, f)
    n_pad = opt['test']['num_pad_front']
    assert opt['test'].get('padding_mode', 'reflect') == 'reflect' and 0 < n_pad
    return yml, n_pad


def test_cli_raw_nv12_in_raw_nv12_out(tmp_path):
    from tecogan_pytorch_amd.models.networks import Yuv
    yml, n_pad = _yml(tmp_path)
    h, w, t = 16, 24, 12
    cfg = ('bt601', True, 'center')
    clip = S.to_semi(planar_clip(t, h, w, '420', 8, 31, cfg), h, w, '420', 8)
    src = str(tmp_path / 'in.nv12')
    open(src, 'wb').write(clip.tobytes())
    r = _cli(['--opt', yml, '--input', src, '--output', '-', '--raw-format', 'nv12', '--raw-size', '24x16',
              '--yuv-matrix', 'bt601', '--yuv-range', 'full', '--yuv-siting', 'center'])
    assert b'nv12 96x64' in r.stderr                                 # the consumer's flags
    spec = Yuv(h, w, '420', None, *cfg, layout='semi')
    assert len(r.stdout) == t * spec.out_frame_bytes(4)             # stdout holds the frames and nothing else
    got = np.frombuffer(r.stdout, np.uint8).reshape(t, spec.out_frame_bytes(4))
    # the model wrapper pads the front; the engine on the padded clip is the reference
    padded = np.concatenate([clip[1:1 + n_pad][::-1], clip], 0)
    ref = streamed(make_net('BD', 4), [padded], spec)[n_pad:]
    assert np.array_equal(got, ref)


def test_cli_raw_p010_in_y4m_444p10_out(tmp_path):
    from tecogan_pytorch_amd.data.y4m import Y4MReader
    yml, n_pad = _yml(tmp_path)
    h, w, t = 16, 24, 12
    cfg = ('bt2020', False, 'left')
    clip = S.to_semi(planar_clip(t, h, w, '420', 10, 32, cfg).view(np.uint16), h, w, '420', 10).view(np.uint8)
    src, raw, y4m = str(tmp_path / 'in.p010'), str(tmp_path / 'out.p410'), str(tmp_path / 'out.y4m')
    open(src, 'wb').write(clip.tobytes())
    common = ['--opt', yml, '--input', src, '--raw-format', 'p010le', '--raw-size', '24x16', '--raw-rate', '30000:1001',
              '--yuv-matrix', 'bt2020', '--output-chroma', '444']
    r = _cli(common + ['--output', raw])
    assert b'p410 96x64' in r.stderr
    _cli(common + ['--output', y4m, '--output-format', 'y4m'])
    rd = Y4MReader(io.BytesIO(open(y4m, 'rb').read()), depths=(8, 10, 12), chromas=('420', '422', '444'))
    assert (rd.w, rd.h, rd.chroma, rd.depth) == (96, 64, '444', 10)
    assert rd.header['tags'] == ['F30000:1001', 'C444p10', 'XYSCSS=444P10']
    planar = np.stack([fr.copy() for fr in rd])
    semi = np.frombuffer(open(raw, 'rb').read(), np.uint8).reshape(t, -1)
    assert planar.shape == semi.shape == (t, 2 * 3 * 64 * 96)
    assert np.array_equal(planar.view(np.uint16), S.to_planar(semi.view(np.uint16), 64, 96, '444', 10))
