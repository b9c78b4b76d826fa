"""Bicubic resize to any size as a specification: MATLAB's contribution algorithm of
tests/bi_ref.py (cubic kernel a = -0.5, stretched when shrinking, normalised weights, indices mirrored with the edge
pixel repeated) with the weights of every output pixel taken to integers over 2^14, so that an 8-bit frame is resized
by one exact integer sum N per output byte and one rounding:

    q    = rint(w * 2^14), the row's residual 2^14 - sum(q) added to its largest q (the first one on a tie)
    N    = sum_r sum_c qv[r] qh[c] x                      (int64, exact)
    byte = clamp((N + 2^27) >> 28, 0, 255)                (floor shift: round-half-up on the exact value)

At the ratios 1/2 and 1/4 the tables are the BI tables times 64 and times 4, and the bytes are bi_downsample_u8's.
Ratios in [1/4, 4] per axis, which bounds the taps per output pixel by MAX_TAPS.  Nothing here has been compared with
MATLAB itself."""
import numpy as np

from tests import bi_ref

WEIGHT_BITS = 14
ONE = 1 << WEIGHT_BITS
MAX_TAPS = 18


def check_sizes(n_in, n_out):
    if n_in < 1 or n_out < 1 or 4 * n_out < n_in or n_out > 4 * n_in:
        raise ValueError(f'resize {n_in} -> {n_out}: both sizes are >= 1 and the ratio lies in [1/4, 4]')


def tables(n_in, n_out):
    """(idx int32 (n_out, P), q int16 (n_out, P)) of one axis: every row of q sums to exactly 2^14."""
    check_sizes(n_in, n_out)
    w, idx = bi_ref.matlab_contributions(n_in, n_out, n_out / n_in)
    q = np.rint(w * ONE).astype(np.int64)
    r = ONE - q.sum(axis=1)
    q[np.arange(n_out), np.argmax(q, axis=1)] += r           # argmax: the first of equal maxima
    assert q.shape[1] <= MAX_TAPS and np.all(q.sum(axis=1) == ONE) and np.abs(q).max() < 2 ** 15
    return np.ascontiguousarray(idx, dtype=np.int32), np.ascontiguousarray(q, dtype=np.int16)


def exact_sums(x_u8, h_out, w_out):
    """The exact integers N (int64) of frames x_u8[..., H, W, 3] -> [..., h_out, w_out, 3]."""
    x = np.asarray(x_u8)
    if x.dtype != np.uint8 or x.ndim < 3 or x.shape[-1] != 3:
        raise ValueError(f'expected uint8 [..., H, W, 3], got {x.dtype} {x.shape}')
    iv, qv = tables(x.shape[-3], h_out)
    ih, qh = tables(x.shape[-2], w_out)
    rows = np.take(x.astype(np.int64), iv, axis=-3)                    # [..., h_out, Pv, W, 3]
    t = np.einsum('ok,...okwc->...owc', qv.astype(np.int64), rows)     # [..., h_out, W, 3]
    cols = np.take(t, ih, axis=-2)                                     # [..., h_out, w_out, Ph, 3]
    return np.einsum('ok,...rokc->...roc', qh.astype(np.int64), cols)  # [..., h_out, w_out, 3]


def round_sums(N):
    return np.clip((N + (1 << (2 * WEIGHT_BITS - 1))) >> (2 * WEIGHT_BITS), 0, 255).astype(np.uint8)


def resize_u8(x_u8, h_out, w_out):
    """uint8 [..., H, W, 3] -> uint8 [..., h_out, w_out, 3]."""
    return round_sums(exact_sums(x_u8, h_out, w_out))


def resize_fp64(x_u8, h_out, w_out):
    """The second formulation: the fp64 weights as they are, rows first, then columns, im2uint8's rounding."""
    x = np.asarray(x_u8).astype(np.float64) / 255.0
    wv, iv = bi_ref.matlab_contributions(x.shape[-3], h_out, h_out / x.shape[-3])
    wh, ih = bi_ref.matlab_contributions(x.shape[-2], w_out, w_out / x.shape[-2])
    t = np.einsum('ok,...okwc->...owc', wv, np.take(x, iv, axis=-3))
    y = np.einsum('ok,...rokc->...roc', wh, np.take(t, ih, axis=-2))
    return np.floor(np.clip(y, 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)


def accumulator_pattern(h_in, w_in, h_out, w_out, oy, ox):
    """The frame (h_in, w_in, 3) that drives output pixel (oy, ox) to its largest sum: 255 where the product of the
    pixel's vertical and horizontal weight is positive, else 0 (mirrored taps that meet on one pixel add up)."""
    iv, qv = tables(h_in, h_out)
    ih, qh = tables(w_in, w_out)
    wv, wh = np.zeros(h_in, np.int64), np.zeros(w_in, np.int64)
    np.add.at(wv, iv[oy], qv[oy].astype(np.int64))
    np.add.at(wh, ih[ox], qh[ox].astype(np.int64))
    x = np.where(np.outer(wv, wh) > 0, 255, 0).astype(np.uint8)
    return np.ascontiguousarray(np.repeat(x[:, :, None], 3, axis=2))
