"""numpy specification of the semi-planar conversions: NV12 / NV16 / NV24 and P010 ... P412 as a
relayout around tests/yuv_planar_ref.py.  Nothing here imports the package.

A semi-planar frame of h x w is the Y plane, then ONE plane of ch rows of 2 cw samples with sample 2c of row r U[r, c]
and sample 2c + 1 V[r, c]; at depth d > 8 a sample is a 16-bit word holding code << (16 - d), read as word >> (16 - d).
Out: the samples are to_semi of the planar specification's.  In: the planar specification on to_planar of the frame."""
import numpy as np

from tests import yuv_planar_ref as P

FORMATS = {'nv12': ('420', 8), 'nv16': ('422', 8), 'nv24': ('444', 8), 'p010': ('420', 10), 'p012': ('420', 12),
           'p210': ('422', 10), 'p212': ('422', 12), 'p410': ('444', 10), 'p412': ('444', 12)}


def to_semi(planar, h, w, chroma, depth):
    """(n, frame_samples) planar codes -> (n, frame_samples) semi-planar samples, written plane by plane."""
    n = planar.shape[0]
    ch, cw = P.chroma_size(h, w, chroma)
    y, u, v = P.planes(planar, h, w, chroma)
    uv = np.stack([u, v], axis=-1)                                  # (n, ch, cw, 2): U then V per chroma sample
    assert uv.shape == (n, ch, cw, 2)
    out = np.concatenate([y.reshape(n, -1), uv.reshape(n, -1)], 1).astype(planar.dtype)
    if depth > 8:
        assert out.dtype == np.uint16 and int(out.max(initial=0)) < (1 << depth)
        out = (out.astype(np.uint32) * (1 << (16 - depth))).astype(np.uint16)
    return out


def to_planar(semi, h, w, chroma, depth):
    """The inverse; the low 16 - depth bits of a word are dropped."""
    n = semi.shape[0]
    ch, cw = P.chroma_size(h, w, chroma)
    y = semi[:, :h * w]
    uv = semi[:, h * w:].reshape(n, ch, cw, 2)
    out = np.concatenate([y, uv[..., 0].reshape(n, -1), uv[..., 1].reshape(n, -1)], 1)
    if depth > 8:
        assert out.dtype == np.uint16
        out = (out.astype(np.uint32) // (1 << (16 - depth))).astype(np.uint16)
    return np.ascontiguousarray(out)


def rgb_u8_to_semi(rgb, chroma, matrix, full_range, siting):
    """(n,H,W,3) uint8 -> (n, frame_bytes) uint8: tg_rgb_u8_to_yuv_semiplanar."""
    H, W = rgb.shape[1:3]
    return to_semi(P.rgb_u8_to_yuv(rgb, chroma, matrix, full_range, siting), H, W, chroma, 8)


def rgb_f32_to_semi(rgb, chroma, depth, matrix, full_range, siting):
    """(n,3,H,W) float32 -> (n, frame_samples) uint16 words: tg_rgb_f32_to_yuv_semiplanar16."""
    H, W = rgb.shape[2:]
    return to_semi(P.rgb_f32_to_yuv(rgb, chroma, depth, matrix, full_range, siting), H, W, chroma, depth)


def semi_to_rgb(semi, h, w, chroma, depth, matrix, full_range, siting):
    """(n, frame_samples) semi-planar samples -> (n,3,h,w) fp64 in [0,1]: the fp64 route of the planar specification."""
    return P.yuv_to_rgb(to_planar(semi, h, w, chroma, depth), h, w, chroma, depth, matrix, full_range, siting)
