"""Synthetic frames for the tOF tests (numpy only, seeded): smooth textures with known sub-pixel motion, and the
contents the kernels' code paths need -- saturated flats, uniform noise, constant frames."""
import numpy as np


def _gauss1d(a, sigma, axis):
    r = int(4 * sigma + 0.5)
    x = np.arange(-r, r + 1, dtype=np.float64)
    t = np.exp(-x * x / (2 * sigma * sigma))
    t /= t.sum()
    pad = np.pad(a, [(r, r) if ax == axis else (0, 0) for ax in range(a.ndim)], mode='reflect')
    n = a.shape[axis]
    return sum(t[i] * (pad[i:i + n] if axis == 0 else pad[:, i:i + n]) for i in range(len(t)))


def smooth_noise(h, w, seed, sigma=2.0):
    """Gaussian-filtered white noise, scaled to [0, 1]."""
    a = np.random.default_rng(seed).standard_normal((h, w))
    a = _gauss1d(_gauss1d(a, sigma, 0), sigma, 1)
    return (a - a.min()) / (a.max() - a.min())


def _cubic_taps(f):
    """Cubic convolution (Keys, a = -0.5) weights of the samples at -1, 0, 1, 2 for the position f in [0, 1)."""
    return np.array([((-0.5 * f + 1.0) * f - 0.5) * f, (1.5 * f - 2.5) * f * f + 1.0,
                     ((-1.5 * f + 2.0) * f + 0.5) * f, (0.5 * f - 0.5) * f * f])


def translate(a, dx, dy):
    """a moved by (dx, dy) pixels (content at x appears at x + dx), cubic interpolation, on the valid interior the
    caller crops: out[y, x] = a(y - dy, x - dx)."""
    out = a
    for axis, d in ((1, dx), (0, dy)):
        s = -d
        i0 = int(np.floor(s))
        t = _cubic_taps(s - i0)
        out = sum(t[k] * np.roll(out, -(i0 - 1 + k), axis=axis) for k in range(4))
    return out


def to_u8(a, gain=255.0, offset=0.0):
    return np.clip(np.rint(a * gain + offset), 0, 255).astype(np.uint8)


def shifted_texture(h, w, shift, seed, margin=32, gain=255.0, offset=0.0):
    """(prev, next) uint8 gray frames of h x w: `next` is `prev` moved by shift = (dx, dy).  gain / offset beyond
    [0, 255] saturate flats into the texture."""
    big = smooth_noise(h + 2 * margin, w + 2 * margin, seed)
    moved = translate(big, shift[0], shift[1])
    crop = (slice(margin, margin + h), slice(margin, margin + w))
    return to_u8(big[crop], gain, offset), to_u8(moved[crop], gain, offset)


def sequence_pair(h, w, t, seed, pred_size=None):
    """(true, pred) uint8 RGB sequences (t, h, w, 3) / (t, *pred_size, 3): a texture that drifts by (1.25, -0.5) px
    per frame; the prediction is the same scene with frame-dependent noise (its flow differs a little)."""
    ph, pw = pred_size or (h, w)
    H, W = max(h, ph), max(w, pw)
    big = smooth_noise(H + 64, W + 64, seed)
    rng = np.random.default_rng(seed + 1000)
    true, pred = [], []
    for i in range(t):
        f = translate(big, 1.25 * i, -0.5 * i)[32:32 + H, 32:32 + W]
        true.append(np.repeat(to_u8(f)[:h, :w, None], 3, 2))
        noisy = f * 255.0 + rng.normal(0.0, 6.0, f.shape)
        pred.append(np.repeat(np.clip(np.rint(noisy), 0, 255).astype(np.uint8)[:ph, :pw, None], 3, 2))
    true, pred = np.stack(true), np.stack(pred)
    true[..., 0] = np.clip(true[..., 0].astype(np.int64) + 9, 0, 255)       # channels differ
    pred[..., 2] = np.clip(pred[..., 2].astype(np.int64) - 7, 0, 255)
    return true, pred
