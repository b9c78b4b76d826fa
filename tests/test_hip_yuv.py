"""Raw YUV 4:2:0 video in and out of the stream on the GPU: the two conversion kernels through the
C ABI against tests/yuv_ref.py -- RGB -> I420 BIT FOR BIT, I420 -> RGB within 5e-7 of fp64 -- at shapes that take every
alignment path (row stride 3W only 2-byte aligned, odd plane offsets, frame strides = 2 mod 4, misaligned base
pointers), with guard bytes around every output; and FRNet.infer_stream(yuv=...) / VSRModel.infer_stream / the CLI,
whose bytes equal rgb_to_yuv420(infer_sequence(yuv420_to_rgb(clip))) bit for bit.

Tolerance of the input direction, 5e-7 absolute (the issue allows 2e-6 and asks for less where a derivation gives it).
The kernel computes yf = ky * (Y - yo) and then one fused multiply-add per chroma term on exact integers (Y - yo and
C16 - 2048 are exact in fp32), with fp32 coefficients rounded from fp64.  Every rounding is at most 2^-24 = 6e-8
relative.  |yf| <= 1.092 carries two of them (ky, the product): 1.3e-7.  B = fma(bu, du, yf): |bu du| <= 1.06 carries
the rounding of bu, 6.3e-8, and the result, at most 2.15, the fma's own, 1.3e-7: 3.2e-7 in all.  R is smaller term by
term.  G = fma(gv, dv, fma(gu, du, yf)): 1.3e-7 (yf) + 1.2e-8 (gu, |gu du| <= 0.2) + 7.7e-8 (inner result <= 1.3) +
2.4e-8 (gv, |gv dv| <= 0.41) + 1.0e-7 (outer result <= 1.7) = 3.5e-7.  The clamp adds nothing."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from procedural_weights import generator_state_dict, smooth_clip
from tests import yuv_ref as R

ROOT_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device('cuda', 0)
GUARD = 0xA5
TOL = 5e-7                                       # see the module docstring
ALL_CONFIGS = [(m, fr, s) for s in R.SITINGS for (m, fr) in R.CONFIGS]          # 2 sitings x 4 matrix / range pairs


def _codes(matrix, full, siting):
    from tecogan_pytorch_amd import _lib as L
    return L.YUV_MATRIX[matrix], int(full), L.YUV_SITING[siting]


def _guarded(nbytes, pad, dtype):
    """A device buffer of `nbytes` payload bytes with `pad` guard bytes on either side, all set to GUARD; the payload
    starts `pad` bytes into a 256-byte aligned allocation (pad 16: aligned for every vector access; pad 1: for none)."""
    buf = torch.full((pad + nbytes + pad,), GUARD, dtype=torch.uint8, device=DEV)
    return buf, buf[pad:pad + nbytes].view(dtype)


def _guards_intact(buf, pad):
    return bool((buf[:pad] == GUARD).all()) and bool((buf[-pad:] == GUARD).all())


def gpu_rgb_to_yuv420(rgb, cfg, pad=16, in_pad=0):
    """tg_rgb_u8_to_yuv420 through the C ABI on (n,H,W,3) uint8 numpy; the input sits in_pad bytes into its buffer."""
    from tecogan_pytorch_amd import _lib as L
    n, H, W, _ = rgb.shape
    src = torch.empty(in_pad + rgb.size, dtype=torch.uint8, device=DEV)
    src[in_pad:].copy_(torch.from_numpy(np.ascontiguousarray(rgb)).reshape(-1))
    buf, out = _guarded(n * R.frame_bytes(H, W), pad, torch.uint8)
    L.check(L.lib().tg_rgb_u8_to_yuv420(src.data_ptr() + in_pad, out.data_ptr(), n, H, W, *_codes(*cfg),
                                        torch.cuda.current_stream().cuda_stream), 'tg_rgb_u8_to_yuv420')
    torch.cuda.synchronize()
    assert _guards_intact(buf, pad), 'tg_rgb_u8_to_yuv420 wrote outside its output'
    return out.cpu().numpy().reshape(n, -1)


def gpu_yuv420_to_rgb(yuv, h, w, cfg, pad=16, in_pad=0):
    """tg_yuv420_to_rgb_f32 through the C ABI on (n, frame_bytes) uint8 numpy -> (n,3,h,w) float32 numpy."""
    from tecogan_pytorch_amd import _lib as L
    n = yuv.shape[0]
    src = torch.empty(in_pad + yuv.size, dtype=torch.uint8, device=DEV)
    src[in_pad:].copy_(torch.from_numpy(np.ascontiguousarray(yuv)).reshape(-1))
    buf, out = _guarded(n * 3 * h * w * 4, pad, torch.float32)
    L.check(L.lib().tg_yuv420_to_rgb_f32(src.data_ptr() + in_pad, out.data_ptr(), n, h, w, *_codes(*cfg),
                                         torch.cuda.current_stream().cuda_stream), 'tg_yuv420_to_rgb_f32')
    torch.cuda.synchronize()
    assert _guards_intact(buf, pad), 'tg_yuv420_to_rgb_f32 wrote outside its output'
    return out.cpu().numpy().reshape(n, 3, h, w)


# ------------------------------------------------------------------ RGB uint8 -> I420: bit identity
def _rgb_inputs(n, H, W, seed):
    rng = np.random.default_rng(seed)
    const = lambda c: np.broadcast_to(np.array(c, np.uint8), (n, H, W, 3)).copy()
    edge = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    edge[:, :, 0] = 255 - edge[:, :, 1]                         # the left column differs from its neighbour
    edge[:, :, 0, 1] = 255
    edge[:, :, 1, 1] = 0
    return {'random': rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8), 'zeros': const((0, 0, 0)),
            'ones': const((255, 255, 255)), 'red': const((255, 0, 0)), 'blue': const((0, 0, 255)), 'left_edge': edge}


@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('H,W', [(2, 2), (4, 6), (18, 18), (16, 34), (18, 258), (64, 96), (6, 8)])
def test_rgb_to_yuv420_is_bit_identical_to_the_integer_specification(H, W, n):
    inputs = _rgb_inputs(n, H, W, seed=H * 1000 + W + n)
    for cfg in ALL_CONFIGS:
        for name, rgb in inputs.items():
            ref = R.rgb_to_yuv420(rgb, *cfg)
            got = gpu_rgb_to_yuv420(rgb, cfg)
            assert got.shape == ref.shape and np.array_equal(got, ref), (cfg, name, int((got != ref).sum()))
    # the full-range clip: pure blue / red reach chroma 256 before it
    for cfg in [c for c in ALL_CONFIGS if c[1]]:
        _, u, _ = R.planes(R.rgb_to_yuv420(inputs['blue'], *cfg), H, W)
        _, _, v = R.planes(R.rgb_to_yuv420(inputs['red'], *cfg), H, W)
        assert (u == 255).all() and (v == 255).all()


@pytest.mark.parametrize('H,W', [(18, 18), (64, 96)])
def test_rgb_to_yuv420_with_misaligned_pointers(H, W):
    """Output and / or input one byte off a dword: the byte-wide form of the kernel, whatever the width."""
    rgb = _rgb_inputs(3, H, W, seed=5)['random']
    for cfg in ALL_CONFIGS:
        ref = R.rgb_to_yuv420(rgb, *cfg)
        for pad, in_pad in ((1, 0), (16, 1), (3, 2)):
            assert np.array_equal(gpu_rgb_to_yuv420(rgb, cfg, pad=pad, in_pad=in_pad), ref), (cfg, pad, in_pad)


# ------------------------------------------------------------------ I420 -> fp32 RGB: 5e-7 of fp64, inside [0,1]
def _yuv_inputs(n, h, w, seed):
    rng = np.random.default_rng(seed)
    ch, cw = (h + 1) // 2, (w + 1) // 2

    def const(y, u, v):
        one = np.concatenate([np.full(h * w, y), np.full(ch * cw, u), np.full(ch * cw, v)]).astype(np.uint8)
        return np.broadcast_to(one, (n, one.size)).copy()
    return {'random': rng.integers(0, 256, (n, R.frame_bytes(h, w)), dtype=np.uint8),
            'out_of_gamut': const(255, 0, 255), 'out_of_gamut_mirror': const(255, 255, 0),
            'below_black': const(0, 255, 0), 'below_black_mirror': const(0, 0, 255)}


@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('h,w', [(2, 2), (8, 8), (9, 11), (13, 34), (9, 9), (16, 258), (3, 5), (4, 6), (6, 8)])
def test_yuv420_to_rgb_is_within_tolerance_of_fp64_and_inside_the_unit_range(h, w, n):
    inputs = _yuv_inputs(n, h, w, seed=h * 1000 + w + n)
    worst = 0.0
    for cfg in ALL_CONFIGS:
        for name, yuv in inputs.items():
            ref = R.yuv420_to_rgb(yuv, h, w, *cfg)
            got = gpu_yuv420_to_rgb(yuv, h, w, cfg)
            assert got.dtype == np.float32 and got.shape == ref.shape
            assert got.min() >= 0.0 and got.max() <= 1.0, (cfg, name)
            err = float(np.abs(got.astype(np.float64) - ref).max())
            worst = max(worst, err)
            assert err <= TOL, (cfg, name, err)
        # Y = 255 with V = 255 is redder than red, with U = 255 bluer than blue: the clamp holds them at exactly 1
        assert (gpu_yuv420_to_rgb(inputs['out_of_gamut'], h, w, cfg)[:, 0] == 1.0).all()
        assert (gpu_yuv420_to_rgb(inputs['out_of_gamut_mirror'], h, w, cfg)[:, 2] == 1.0).all()
    print('worst |gpu - fp64| at %dx%d n=%d: %.3g' % (h, w, n, worst))


@pytest.mark.parametrize('h,w', [(9, 11), (8, 8)])
def test_yuv420_to_rgb_with_misaligned_pointers(h, w):
    yuv = _yuv_inputs(3, h, w, seed=6)['random']
    for cfg in ALL_CONFIGS:
        ref = R.yuv420_to_rgb(yuv, h, w, *cfg)
        for pad, in_pad in ((4, 0), (16, 1), (8, 3)):              # (the output is fp32: guards in whole floats)
            got = gpu_yuv420_to_rgb(yuv, h, w, cfg, pad=pad, in_pad=in_pad)
            assert float(np.abs(got - ref).max()) <= TOL, (cfg, pad, in_pad)


def test_ops_wrappers_equal_the_c_abi_and_refuse_cpu_tensors():
    from tecogan_pytorch_amd import _lib as L, ops
    rgb = _rgb_inputs(2, 16, 34, seed=1)['random']
    yuv = _yuv_inputs(2, 9, 11, seed=1)['random']
    for cfg in (('bt709', False, 'left'), ('bt601', True, 'center')):
        got = ops.rgb_to_yuv420(torch.from_numpy(rgb).to(DEV), *cfg)
        assert got.shape == (2, R.frame_bytes(16, 34)) and np.array_equal(got.cpu().numpy(), R.rgb_to_yuv420(rgb, *cfg))
        back = ops.yuv420_to_rgb(torch.from_numpy(yuv).to(DEV), 9, 11, *cfg)
        assert back.shape == (2, 3, 9, 11) and np.array_equal(back.cpu().numpy(), gpu_yuv420_to_rgb(yuv, 9, 11, cfg))
        one = ops.yuv420_to_rgb(torch.from_numpy(yuv[0]).to(DEV), 9, 11, *cfg)
        assert torch.equal(one, back[:1])
    assert np.array_equal(ops.rgb_to_yuv420(torch.from_numpy(rgb).to(DEV)).cpu().numpy(),
                          R.rgb_to_yuv420(rgb, 'bt709', False, 'left'))                   # the defaults
    with pytest.raises(L.TecoganHipError):
        ops.rgb_to_yuv420(torch.from_numpy(rgb))
    with pytest.raises(L.TecoganHipError):
        ops.yuv420_to_rgb(torch.from_numpy(yuv), 9, 11)
    with pytest.raises(L.TecoganHipError):
        ops.yuv420_to_rgb(torch.from_numpy(yuv).to(DEV), 9, 12)                          # the size does not match


def test_both_ops_return_tg_e_arg_without_a_launch():
    from tecogan_pytorch_amd import _lib as L, ops
    lib = L.lib()
    rgb = torch.zeros(1, 6, 6, 3, dtype=torch.uint8, device=DEV)
    yuv = torch.full((R.frame_bytes(6, 6),), GUARD, dtype=torch.uint8, device=DEV)
    out = torch.full((3 * 6 * 6,), 7.0, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    E_ARG = -2
    # odd H / W in the output direction
    assert lib.tg_rgb_u8_to_yuv420(rgb.data_ptr(), yuv.data_ptr(), 1, 5, 6, 1, 0, 1, st) == E_ARG
    assert lib.tg_rgb_u8_to_yuv420(rgb.data_ptr(), yuv.data_ptr(), 1, 6, 5, 1, 0, 1, st) == E_ARG
    assert b'even' in lib.tg_last_error_string()
    # unknown enum values, n = 0, null pointers
    for m, r, s in ((2, 0, 0), (-1, 0, 0), (0, 2, 0), (0, -1, 0), (0, 0, 2), (1, 1, -1)):
        assert lib.tg_rgb_u8_to_yuv420(rgb.data_ptr(), yuv.data_ptr(), 1, 6, 6, m, r, s, st) == E_ARG
        assert lib.tg_yuv420_to_rgb_f32(yuv.data_ptr(), out.data_ptr(), 1, 6, 6, m, r, s, st) == E_ARG
    assert lib.tg_rgb_u8_to_yuv420(rgb.data_ptr(), yuv.data_ptr(), 0, 6, 6, 1, 0, 1, st) == E_ARG
    assert lib.tg_yuv420_to_rgb_f32(yuv.data_ptr(), out.data_ptr(), 0, 6, 6, 1, 0, 1, st) == E_ARG
    assert lib.tg_rgb_u8_to_yuv420(None, yuv.data_ptr(), 1, 6, 6, 1, 0, 1, st) == E_ARG
    assert lib.tg_yuv420_to_rgb_f32(yuv.data_ptr(), None, 1, 6, 6, 1, 0, 1, st) == E_ARG
    assert lib.tg_yuv420_to_rgb_f32(yuv.data_ptr(), out.data_ptr(), 1, 1, 6, 1, 0, 1, st) == E_ARG
    torch.cuda.synchronize()
    assert bool((yuv == GUARD).all()) and bool((out == 7.0).all()), 'a refused call launched'
    # and through the wrappers: TecoganHipError
    with pytest.raises(L.TecoganHipError, match='code -2'):
        ops.rgb_to_yuv420(torch.zeros(1, 5, 6, 3, dtype=torch.uint8, device=DEV))
    with pytest.raises(L.TecoganHipError, match='code -2'):
        ops.rgb_to_yuv420(rgb, matrix=7)
    with pytest.raises(L.TecoganHipError, match='code -2'):
        ops.yuv420_to_rgb(yuv, 6, 6, siting=5)
    with pytest.raises(L.TecoganHipError, match='code -2'):
        ops.rgb_to_yuv420(torch.zeros(0, 6, 6, 3, dtype=torch.uint8, device=DEV))
    with pytest.raises(L.TecoganHipError, match='code -2'):
        ops.yuv420_to_rgb(torch.zeros(0, R.frame_bytes(6, 6), dtype=torch.uint8, device=DEV), 6, 6)
    with pytest.raises(L.TecoganHipError):
        ops.rgb_to_yuv420(rgb, matrix='bt2020')


# ------------------------------------------------------------------ the stream
def make_net(deg, s, precision='fp32'):
    from tecogan_pytorch_amd.models.networks import FRNet
    net = FRNet(3, 3, 64, 10, deg, s, precision=precision)
    net.load_state_dict(generator_state_dict(scale=s, degradation=deg), strict=True)
    return net.cuda().eval()


@pytest.fixture(scope='module')
def net4():
    return make_net('BD', 4)


def i420_clip(t, h, w, seed, matrix='bt709', full=False, siting='left'):
    """(t, frame_bytes) uint8: a smooth moving clip converted by the integer specification at the even size that
    covers h x w, its Y plane cropped to h x w (odd sizes keep ceil(h/2) x ceil(w/2) chroma)."""
    he, we = 2 * ((h + 1) // 2), 2 * ((w + 1) // 2)
    clip = smooth_clip(t, 3, he, we, seed=seed)
    u8 = (clip.permute(0, 2, 3, 1) * 255.0).round().clamp(0, 255).to(torch.uint8).numpy()
    y, u, v = R.planes(R.rgb_to_yuv420(u8, matrix, full, siting), he, we)
    return np.ascontiguousarray(np.concatenate([y[:, :h, :w].reshape(t, -1), u.reshape(t, -1), v.reshape(t, -1)], 1))


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


def reference(net, clip, spec):
    """rgb_to_yuv420(infer_sequence(yuv420_to_rgb(clip))): the two ops around the frames the stream yields today."""
    from tecogan_pytorch_amd import ops
    cfg = (spec.matrix, spec.full_range, spec.siting)
    lr = ops.yuv420_to_rgb(torch.from_numpy(clip).to(DEV), spec.h, spec.w, *cfg)
    hr = net.infer_sequence(lr.cpu(), DEV)
    assert hr.shape == (len(clip), net.scale * spec.h, net.scale * spec.w, 3)
    return ops.rgb_to_yuv420(torch.from_numpy(np.ascontiguousarray(hr)).to(DEV), *cfg).cpu().numpy()


@pytest.mark.parametrize('t', [1, 10, 30])
@pytest.mark.parametrize('h,w,cfg', [(16, 24, ('bt709', False, 'left')), (9, 11, ('bt601', True, 'center'))])
def test_yuv_stream_equals_the_ops_around_infer_sequence_bit_for_bit(net4, h, w, cfg, t):
    from tecogan_pytorch_amd.models.networks import Yuv420
    spec = Yuv420(h, w, *cfg)
    clip = i420_clip(t, h, w, 40 + t, *cfg)
    ref = reference(net4, clip, spec)
    assert ref.shape == (t, spec.out_frame_bytes(4))
    for name, items in chunkings(clip).items():
        got = streamed(net4, items, spec)
        assert got.shape == ref.shape and np.array_equal(got, ref), (name, int((got != ref).sum()))
    if t == 30:                                                     # torch items as well, and the chunks are the engine's
        sizes = [len(c) for c in net4.infer_stream(iter([torch.from_numpy(clip)]), DEV, yuv=spec)]
        assert sizes == [9, 8, 8, 5]


def test_yuv_stream_2x_bi():
    from tecogan_pytorch_amd.models.networks import Yuv420
    net = make_net('BI', 2)
    spec = Yuv420(9, 11, 'bt709', True, 'left')
    clip = i420_clip(19, 9, 11, 8, 'bt709', True, 'left')
    ref = reference(net, clip, spec)
    assert ref.shape == (19, 18 * 22 * 3 // 2)
    assert np.array_equal(streamed(net, chunkings(clip)['uneven'], spec), ref)


def test_yuv_stream_fp16():
    from tecogan_pytorch_amd.models.networks import Yuv420
    net = make_net('BD', 4, precision='fp16')
    spec = Yuv420(16, 24, 'bt601', False, 'center')
    clip = i420_clip(21, 16, 24, 9, 'bt601', False, 'center')
    assert np.array_equal(streamed(net, chunkings(clip)['uneven'], spec), reference(net, clip, spec))
    assert net._get_plan(1, 16, 24, DEV).precision == 'fp16'


def test_yuv_stream_full_size_uses_the_resident_launch(net4):
    import ctypes
    from tecogan_pytorch_amd import _lib
    from tecogan_pytorch_amd.models.networks import Yuv420
    spec = Yuv420(134, 320)
    clip = i420_clip(12, 134, 320, 2)
    ref = reference(net4, clip, spec)
    assert np.array_equal(streamed(net4, chunkings(clip)['uneven'], spec), ref)
    lib = _lib.lib()
    plan = net4._get_plan(1, 134, 320, DEV)
    names = [lib.tg_frnet_kind_name(k).decode() for k in range(lib.tg_frnet_plan_kinds())]
    nl = ctypes.c_int()
    _lib.check(lib.tg_frnet_plan_kind_stats(plan.handle, names.index('conv3x3_wino_resident_kernel'), ctypes.byref(nl),
                                            None, None), 'kind_stats')
    assert nl.value == 1 and plan.chain_state() == (0, True)


def test_yuv_stream_refuses_bad_items_and_stays_usable(net4):
    from tecogan_pytorch_amd.models.networks import Yuv420
    spec = Yuv420(16, 24)
    clip = i420_clip(20, 16, 24, 3)
    ref = reference(net4, clip, spec)
    for bad in (np.zeros(spec.frame_bytes + 1, np.uint8), clip[0].astype(np.float32), torch.from_numpy(clip[:2]).to(DEV),
                np.zeros((16, 24, 3), np.uint8)):
        got = []
        with pytest.raises(ValueError, match='infer_stream'):
            for chunk in net4.infer_stream(iter([f for f in clip[:12]] + [bad]), DEV, yuv=spec):
                got.append(chunk.copy())
        if got:
            assert np.array_equal(np.concatenate(got, 0), ref[:sum(len(c) for c in got)])
    assert np.array_equal(streamed(net4, [clip], spec), ref)


def test_yielded_yuv_chunk_is_valid_until_the_generator_is_advanced(net4):
    from tecogan_pytorch_amd.models.networks import Yuv420, yuv420_planes
    spec = Yuv420(16, 24)
    clip = i420_clip(60, 16, 24, 3)
    ref = reference(net4, clip, spec)
    pos = 0
    for chunk in net4.infer_stream(iter(chunkings(clip)['frames']), DEV, yuv=spec):
        mine = chunk.copy()
        torch.cuda.synchronize()                 # every batch in flight has finished, downloads included
        assert np.array_equal(chunk, mine), 'a batch in flight wrote into the slot the caller holds'
        assert np.array_equal(mine, ref[pos:pos + len(mine)])
        y, u, v = yuv420_planes(chunk, 64, 96)
        assert y.shape == (len(mine), 64, 96) and u.shape == v.shape == (len(mine), 32, 48) and np.shares_memory(y, chunk)
        pos += len(mine)
    assert pos == 60


def test_yuv_stream_host_buffer_may_be_reused_by_the_caller(net4):
    from tecogan_pytorch_amd.models.networks import Yuv420
    spec = Yuv420(16, 24)
    clip = i420_clip(20, 16, 24, 6)
    ref = reference(net4, clip, spec)
    buf = np.empty(spec.frame_bytes, np.uint8)

    def source():
        for i in range(20):
            buf[:] = clip[i]
            yield buf
    assert np.array_equal(streamed(net4, source(), spec), ref)


def test_yuv_stream_memory_does_not_grow_with_the_length(net4):
    from tecogan_pytorch_amd.models.networks import Yuv420
    spec = Yuv420(16, 24)
    base = i420_clip(10, 16, 24, 7)

    def run(t):
        n = 0
        for chunk in net4.infer_stream((base[i % 10] for i in range(t)), DEV, yuv=spec):
            n += len(chunk)
        assert n == t
    for t in (30, 120):                          # plans of every batch size exist before anything is measured
        run(t)
    peaks = []
    for t in (30, 120):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        run(t)
        torch.cuda.synchronize()
        peaks.append(torch.cuda.max_memory_allocated())
    print('device peaks of a 30- and a 120-frame yuv stream:', peaks)
    assert peaks[0] == peaks[1], peaks


# ------------------------------------------------------------------ the model wrapper and the CLI
def _opt(n_pad=5):
    from tecogan_pytorch_amd.main import default_opt
    opt = default_opt()
    opt.update({'is_train': False, 'dist': False, 'device': 'cuda', 'rank': 0, 'world_size': 1})
    opt['test']['num_pad_front'] = n_pad
    return opt


def test_vsr_model_infer_stream_pads_i420_items():
    from tecogan_pytorch_amd.models import define_model
    from tecogan_pytorch_amd.models.networks import Yuv420
    model = define_model(_opt(n_pad=2))
    model.net_G.load_state_dict(generator_state_dict(scale=4, degradation='BD'), strict=True)
    spec = Yuv420(16, 24)
    clip = i420_clip(13, 16, 24, 21)
    padded = np.concatenate([clip[1:3][::-1], clip], 0)             # reflect, num_pad_front = 2
    ref = streamed(model.net_G, [padded], spec)[2:]
    for items in ([f for f in clip], [clip[:1], clip[1:2], clip[2:]], [torch.from_numpy(clip)]):
        got = np.concatenate([c.copy() for c in model.infer_stream(iter(items), yuv=spec)], 0)
        assert got.shape == ref.shape == (13, spec.out_frame_bytes(4)) and np.array_equal(got, ref)
    with pytest.raises(ValueError, match='at least 3'):
        list(model.infer_stream(iter([clip[:2]]), yuv=spec))


def test_cli_y4m_in_y4m_out_and_stdout_holds_nothing_else(tmp_path):
    import yaml
    from tecogan_pytorch_amd import main as M
    from tecogan_pytorch_amd.data.y4m import Y4MReader
    from tecogan_pytorch_amd.models import define_model
    from tecogan_pytorch_amd.models.networks import Yuv420
    pth = str(tmp_path / 'G_iter7.pth')
    torch.save(generator_state_dict(scale=4, degradation='BD'), pth)
    opt = M.default_opt()
    opt['model']['generator']['load_path'] = pth
    yml = str(tmp_path / 'infer.yml')
    with open(yml, 'w') as f:
        yaml.safe_dump(opt, f)
    h, w, t = 16, 24, 12
    clip = i420_clip(t, h, w, 31, 'bt601', True, 'center')
    src, dst = str(tmp_path / 'in.y4m'), str(tmp_path / 'out.y4m')
    with open(src, 'wb') as f:
        f.write(b'YUV4MPEG2 W24 H16 F25:1 Ip A1:1 C420jpeg XYSCSS=420JPEG XCOLORRANGE=FULL\n')
        for fr in clip:
            f.write(b'FRAME\n' + fr.tobytes())
    M.main(['--mode', 'infer', '--opt', yml, '--input', src, '--output', dst, '--yuv-matrix', 'bt601'])
    data = open(dst, 'rb').read()
    rd = Y4MReader(io.BytesIO(data))
    assert (rd.w, rd.h, rd.siting, rd.full_range) == (96, 64, 'center', True)
    assert rd.header['tags'] == ['F25:1', 'A1:1', 'C420jpeg', 'XYSCSS=420JPEG', 'XCOLORRANGE=FULL']
    got = np.stack([fr.copy() for fr in rd])
    ref_opt = _opt()
    ref_opt['model']['generator']['load_path'] = pth
    model = define_model(ref_opt)
    spec = Yuv420(h, w, 'bt601', True, 'center')                    # (the range comes from the header)
    api = np.concatenate([c.copy() for c in model.infer_stream(iter([f for f in clip]), yuv=spec)], 0)
    assert got.shape == api.shape == (t, spec.out_frame_bytes(4)) and np.array_equal(got, api)
    # --output -: a fresh process whose stdout is the y4m stream and nothing else; stdin feeds it
    env = dict(os.environ, PYTHONPATH=ROOT_DIR + os.pathsep + os.environ.get('PYTHONPATH', ''))
    r = subprocess.run([sys.executable, '-m', 'tecogan_pytorch_amd.main', '--mode', 'infer', '--opt', yml, '--input', '-',
                        '--output', '-', '--yuv-matrix', 'bt601'], input=open(src, 'rb').read(), cwd=ROOT_DIR, env=env,
                       capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout == data, (len(r.stdout), len(data), r.stdout[:80])
    assert b'12 frames' in r.stderr
