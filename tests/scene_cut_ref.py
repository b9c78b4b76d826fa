"""numpy restatement of the scene-cut detector (include/tecogan_hip.h).  The formula is the
specification: everything after the one fp32 rounding of fma(x, 255, 0.5) is integer arithmetic, so the device must
give these numbers bit for bit."""
import math

import numpy as np

BINS = 32
MAD, HIST = 24.0, 0.25                          # the defaults of SceneCut


def quant255(x):
    """clamp(floor(fma(x, 255, 0.5)), 0, 255), NaN -> 0.  x * 255 is exact in fp64 (24 + 8 bits) and so is the sum for
    every x that matters, so rounding the fp64 value to fp32 once is the fused multiply-add."""
    x = np.asarray(x, np.float32)
    with np.errstate(over='ignore', invalid='ignore'):
        v = np.floor((x.astype(np.float64) * 255.0 + 0.5).astype(np.float32))
    v = np.where(np.isnan(v), np.float32(0), v)
    return np.clip(v, 0, 255).astype(np.int64)


def luma(frames):
    """(..., 3, h, w) fp32 -> (..., h, w) int64 in 0..255."""
    q = quant255(frames)
    return (77 * q[..., 0, :, :] + 150 * q[..., 1, :, :] + 29 * q[..., 2, :, :] + 128) >> 8


def thresholds(mad, hist, h, w):
    """(S_min, D_min): what the host hands to the device."""
    n = h * w
    return math.ceil(mad * n), math.ceil(hist * 2 * n)


def stats(frames):
    """frames (n + 1, 3, h, w) -> (sad (n,), hdist (n,)) int64: pair j is frame j + 1 against frame j."""
    y = luma(np.asarray(frames))
    sad = np.abs(y[1:] - y[:-1]).reshape(len(y) - 1, -1).sum(1)
    hg = np.stack([np.bincount((f >> 3).ravel(), minlength=BINS) for f in y]).astype(np.int64)
    return sad, np.abs(hg[1:] - hg[:-1]).sum(1)


def flags(frames, s_min, d_min, forced=None, detect=True):
    """-> (flags (n,) int32, sad (n,) uint64, hdist (n,) uint32)."""
    sad, hd = stats(frames)
    f = np.zeros(len(sad), bool) if forced is None else np.asarray(forced).astype(bool)
    if detect:
        f = f | ((sad >= s_min) & (hd >= d_min))
    return f.astype(np.int32), sad.astype(np.uint64), hd.astype(np.uint32)


def stream_cuts(clip, mad=MAD, hist=HIST, detect=True, at=()):
    """What a stream over `clip` (t, 3, h, w) reports: (cuts, scores) with scores[i] = (S_i / N, D_i / 2N) of frame i
    against frame i - 1, the frame before frame 0 being zeros.  Frame 0 is never a cut."""
    clip = np.asarray(clip, np.float32)
    t, _, h, w = clip.shape
    s_min, d_min = thresholds(mad, hist, h, w)
    forced = np.zeros(t, np.uint8)
    for a in at:
        if 0 <= a < t:
            forced[a] = 1
    f, sad, hd = flags(np.concatenate([np.zeros_like(clip[:1]), clip], 0), s_min, d_min, forced, detect)
    n = h * w
    return ([i for i in range(1, t) if f[i]],
            [(int(sad[i]) / n, int(hd[i]) / (2 * n)) for i in range(t)])
