"""Semi-planar YUV: NV12 / NV16 / NV24 at 8 bits, P010 / P012, P210 / P212, P410 / P412 above --
a Y plane followed by ONE plane of interleaved U,V pairs, and above 8 bits the code in the top bits of a 16-bit word.
Tensor-level wrappers over the three semi-planar entry points, built on the bodies of ops (ops._call, ops._yuv_in,
ops._yuv_out), so the boundary rule of ops holds here as well: every tensor is checked for device, dtype and contiguity
before anything is allocated or reaches the library.  And the relayout between the planar and the semi-planar form of
a frame in numpy, for callers that hold one and need the other.

A frame has the samples of the planar frame of the same chroma (ops.yuv_frame_samples), and the values are the planar
wrappers' (ops.yuv_to_rgb, ops.rgb_to_yuv, ops.rgb_f32_to_yuv) on the relaid frame, bit for bit."""
import numpy as np
import torch

from . import _lib as L
from . import ops
from .ops import YUV_SUBSAMPLING, yuv_frame_samples


def _sizes(frames, h, w, chroma, depth, who):
    if chroma not in YUV_SUBSAMPLING:
        raise ValueError(f'{who}: chroma is one of {sorted(YUV_SUBSAMPLING)}, got {chroma!r}')
    if depth not in (8, 10, 12):
        raise ValueError(f'{who}: depth is 8, 10 or 12, got {depth!r}')
    sx, sy = YUV_SUBSAMPLING[chroma]
    ch, cw = (h + sy - 1) // sy, (w + sx - 1) // sx
    frames = np.asarray(frames)
    want = np.uint8 if depth == 8 else np.uint16
    if frames.dtype != want or frames.ndim not in (1, 2) or frames.shape[-1] != h * w + 2 * ch * cw:
        raise ValueError(f'{who}: {h}x{w} {chroma} frames at {depth} bits are {np.dtype(want).name} (n, '
                         f'{h * w + 2 * ch * cw}); got {frames.dtype} {frames.shape}')
    return frames, h * w, ch * cw


def to_semi(planar, h, w, chroma='420', depth=8):
    """(n, frame_samples) / (frame_samples,) planar frames (Y, U, V; uint8 at depth 8, uint16 codes above) -> the
    semi-planar frames of the same shape: Y, then U and V interleaved, every 16-bit sample shifted left by 16 - depth."""
    planar, ny, nc = _sizes(planar, h, w, chroma, depth, 'to_semi')
    out = np.empty_like(planar)
    out[..., :ny] = planar[..., :ny]
    out[..., ny::2] = planar[..., ny:ny + nc]
    out[..., ny + 1::2] = planar[..., ny + nc:]
    return out if depth == 8 else out << np.uint16(16 - depth)


def to_planar(semi, h, w, chroma='420', depth=8):
    """The inverse of to_semi: every 16-bit word shifted right by 16 - depth (its low bits are dropped), U and V
    separated into planes."""
    semi, ny, nc = _sizes(semi, h, w, chroma, depth, 'to_planar')
    out = np.empty_like(semi)
    out[..., :ny] = semi[..., :ny]
    out[..., ny:ny + nc] = semi[..., ny::2]
    out[..., ny + nc:] = semi[..., ny + 1::2]
    return out if depth == 8 else out >> np.uint16(16 - depth)


def to_rgb(yuv, h, w, chroma='420', depth=8, matrix='bt709', full_range=False, siting='left', out=None):
    """(n, frame_samples) / (frame_samples,) semi-planar frames on device -- uint8 at depth 8, uint16 words at 10 | 12
    -- -> (n,3,h,w) fp32 RGB in [0,1] (tg_yuv_semiplanar_to_rgb_f32): ops.yuv_to_rgb of the relaid frames, bit for
    bit.  out: a contiguous CUDA float32 (n,3,h,w) tensor to write into."""
    ops._chk_depth(depth, 'semiplanar.to_rgb', '8, 10 or 12')
    c, m, r, s = ops._yuv_codes('semiplanar.to_rgb', L.YUV_PLANAR_MATRIX, matrix, full_range, siting, chroma)
    chroma = {v: k for k, v in L.YUV_CHROMA.items()}.get(c)          # (None: the library refuses it before any access)
    ns = None if chroma is None else yuv_frame_samples(h, w, chroma)
    return ops._yuv_in('semiplanar.to_rgb', 'tg_yuv_semiplanar_to_rgb_f32', yuv,
                       torch.uint8 if depth == 8 else torch.uint16, h, w, ns,
                       f'semi-planar {chroma} frames have {ns} samples', (c, depth, m, r, s), out)


def from_rgb(rgb_hwc, chroma='420', matrix='bt709', full_range=False, siting='left'):
    """(n,H,W,3) uint8 RGB on device -> (n, frame_samples) uint8 semi-planar frames (nv12 | nv16 | nv24), exact integer
    arithmetic (tg_rgb_u8_to_yuv_semiplanar).  '420': H and W even; '422': W even; '444': any size."""
    if not isinstance(chroma, str):
        raise L.TecoganHipError(f'semiplanar.from_rgb: chroma is one of {sorted(L.YUV_CHROMA)}, got {chroma!r}')
    return ops._yuv_out('semiplanar.from_rgb', 'tg_rgb_u8_to_yuv_semiplanar', rgb_hwc, False, chroma,
                        ops._yuv_codes('semiplanar.from_rgb', L.YUV_PLANAR_MATRIX, matrix, full_range, siting, chroma))


def from_rgb_f32(rgb_chw, chroma='420', depth=10, matrix='bt709', full_range=False, siting='left', out=None):
    """(n,3,H,W) float32 RGB on device -> (n, frame_samples) uint16 semi-planar frames at `depth` (10 | 12) bits, the
    code in the top bits of every word (tg_rgb_f32_to_yuv_semiplanar16).  The sizes of from_rgb.  out: a contiguous CUDA
    uint16 (n, frame_samples) tensor to write into."""
    if not isinstance(chroma, str):
        raise L.TecoganHipError(f'semiplanar.from_rgb_f32: chroma is one of {sorted(L.YUV_CHROMA)}, got {chroma!r}')
    c, m, r, s = ops._yuv_codes('semiplanar.from_rgb_f32', L.YUV_PLANAR_MATRIX, matrix, full_range, siting, chroma)
    return ops._yuv_out('semiplanar.from_rgb_f32', 'tg_rgb_f32_to_yuv_semiplanar16', rgb_chw, True, chroma,
                        (c, ops._chk_depth(depth, 'semiplanar.from_rgb_f32'), m, r, s), out)
