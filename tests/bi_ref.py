"""The BI degradation as a specification: what scripts/generate_lr_bi.m of the reference does
to an 8-bit frame -- im2double, modcrop, imresize(img, 1/s, 'bicubic'), imwrite -- restated in integers.

For s in {2, 4} and sizes that are multiples of s, MATLAB's contribution algorithm (cubic kernel, a = -0.5, stretched
by s, weights normalised, indices mirrored with the edge pixel repeated) gives every output pixel the same T = 4s
weights, dyadic rationals that sum to exactly 1: WEIGHTS[s] / DENOM[s].  With 8-bit input the whole degradation is
then one exact integer sum N per output byte and one rounding:

    byte = clamp((2 N + D) // (2 D), 0, 255),   D = DENOM[s] ** 2

i.e. round-half-up on the exact value.  (MATLAB decides an exact tie by the rounding noise of its double-precision
sums; the tie rule here is a decision of this project.)  `matlab_contributions` is the general algorithm in fp64, kept
as the second formulation tests/test_bi_ref_cpu.py compares the tables and the integer route with.  Nothing here has
been compared with MATLAB itself."""
import numpy as np

_HALF = {2: (-3, -9, 29, 111), 4: (-7, -45, -75, -49, 93, 399, 745, 987)}
WEIGHTS = {s: np.array(h + h[::-1], dtype=np.int64) for s, h in _HALF.items()}
DENOM = {2: 256, 4: 4096}
BORDER_LR = 2            # pad=False: the input carries 2 s GT pixels per side = 2 LR pixels cut from every side


def mirror_index(i, n):
    """MATLAB's aux = [1:n, n:-1:1]; aux(mod(i - 1, 2 n) + 1) on 0-based indices: the edge pixel is repeated
    (numpy's 'symmetric'), as often as the halo needs."""
    i = np.mod(np.asarray(i, dtype=np.int64), 2 * n)
    return np.where(i < n, i, 2 * n - 1 - i)


def tap_indices(n, s):
    """(n // s, 4 s): the input pixels output pixel o reads along an axis of n pixels (n a multiple of s)."""
    o = np.arange(n // s, dtype=np.int64)[:, None]
    return mirror_index(s * o - 3 * s // 2 + np.arange(4 * s, dtype=np.int64)[None, :], n)


def exact_sums(x_u8, s):
    """The exact integers N (int64) of the modcropped frames x_u8[..., H, W, 3] -> [..., H/s, W/s, 3]."""
    if s not in WEIGHTS:
        raise ValueError(f'scale {s}: the BI degradation is specified for 2 and 4')
    x = np.asarray(x_u8)
    if x.dtype != np.uint8 or x.ndim < 3 or x.shape[-1] != 3:
        raise ValueError(f'expected uint8 [..., H, W, 3], got {x.dtype} {x.shape}')
    H, W = x.shape[-3], x.shape[-2]
    hc, wc = H - H % s, W - W % s
    if hc < s or wc < s:
        raise ValueError(f'{H}x{W} is smaller than one {s}x{s} block')
    x = x[..., :hc, :wc, :].astype(np.int64)
    k = WEIGHTS[s]
    rows = np.take(x, tap_indices(hc, s), axis=-3)                    # [..., H/s, T, W, 3]
    t = np.tensordot(rows, k, axes=([-3], [0]))                       # [..., H/s, W, 3]
    cols = np.take(t, tap_indices(wc, s), axis=-2)                    # [..., H/s, W/s, T, 3]
    return np.tensordot(cols, k, axes=([-2], [0]))                    # [..., H/s, W/s, 3]


def round_sums(N, s):
    D = DENOM[s] ** 2
    return np.clip((2 * N + D) // (2 * D), 0, 255).astype(np.uint8)


def is_tie(N, s):
    """Outputs whose exact value lies on k + 1/2: found from the integers alone."""
    D = DENOM[s] ** 2
    return (2 * N + D) % (2 * D) == 0


def bi_downsample_u8(x_u8, s, pad=True):
    """uint8 [..., H, W, 3] -> uint8 [..., H', W', 3].  pad=True (test time): H' = (H - H % s) / s, mirrored borders.
    pad=False (training): the same with BORDER_LR pixels cut from every side -- no mirrored tap is read."""
    y = round_sums(exact_sums(x_u8, s), s)
    if pad:
        return y
    b = BORDER_LR
    if y.shape[-3] <= 2 * b or y.shape[-2] <= 2 * b:
        raise ValueError(f'pad=False needs more than {4 * s} pixels per axis, got {np.asarray(x_u8).shape}')
    return np.ascontiguousarray(y[..., b:-b, b:-b, :])


def bi_lr_float(y_u8):
    """uint8 [..., H, W, 3] -> float32 [..., 3, H, W]: the values the loaders make of an LR PNG."""
    y = np.asarray(y_u8)
    return np.ascontiguousarray(np.moveaxis(y.astype(np.float32) / np.float32(255), -1, -3))


# ---- second formulation: the general contribution algorithm, fp64 --------------------------------------------------
def _cubic(x):
    ax = np.abs(x)
    ax2, ax3 = ax * ax, ax * ax * ax
    return (1.5 * ax3 - 2.5 * ax2 + 1) * (ax <= 1) + (-0.5 * ax3 + 2.5 * ax2 - 4 * ax + 2) * ((1 < ax) & (ax <= 2))


def matlab_contributions(n_in, n_out, scale):
    """imresize's contributions(): weights (n_out, P) fp64 and 0-based indices (n_out, P) into the input axis."""
    kernel_width = 4.0
    if scale < 1:
        def h(x):
            return scale * _cubic(scale * x)
        kernel_width = kernel_width / scale
    else:
        h = _cubic
    x = np.arange(1, n_out + 1, dtype=np.float64)
    u = x / scale + 0.5 * (1 - 1 / scale)
    left = np.floor(u - kernel_width / 2)
    P = int(np.ceil(kernel_width)) + 2
    indices = left[:, None] + np.arange(P, dtype=np.float64)[None, :]
    weights = h(u[:, None] - indices)
    weights = weights / weights.sum(axis=1, keepdims=True)
    aux = np.concatenate([np.arange(1, n_in + 1), np.arange(n_in, 0, -1)])
    indices = aux[np.mod(indices.astype(np.int64) - 1, 2 * n_in)]
    keep = np.any(weights != 0, axis=0)
    return weights[:, keep], indices[:, keep] - 1


def resize_fp64(img, s):
    """img [H, W, C] fp64 (already modcropped) through the contributions, rows first, then columns."""
    H, W = img.shape[:2]
    wv, iv = matlab_contributions(H, H // s, 1.0 / s)
    wh, ih = matlab_contributions(W, W // s, 1.0 / s)
    t = np.einsum('ok,okwc->owc', wv, img[iv])
    return np.einsum('ok,rokc->roc', wh, t[:, ih])


def bi_downsample_fp64(x_u8, s):
    """The .m file's route in fp64: im2double, modcrop, imresize, im2uint8."""
    x = np.asarray(x_u8)
    H, W = x.shape[:2]
    y = resize_fp64(x[:H - H % s, :W - W % s].astype(np.float64) / 255.0, s)
    return np.floor(np.clip(y, 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)
