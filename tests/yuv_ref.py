"""numpy restatement of the two I420 conversions, shared by tests/test_yuv_cpu.py and
tests/test_hip_yuv.py.  Nothing here imports the package: the integer output direction is the SPECIFICATION (the GPU must
equal rgb_to_yuv420 bit for bit), the input direction is stated in fp64 (the GPU's fp32 step must be within 2e-6)."""
import numpy as np

KR_KB = {'bt601': (0.299, 0.114), 'bt709': (0.2126, 0.0722)}
CONFIGS = [(m, fr) for m in ('bt601', 'bt709') for fr in (False, True)]
SITINGS = ('center', 'left')


def scales(full_range):
    """(yo, ys, cs)"""
    return (0, 255.0, 255.0) if full_range else (16, 219.0, 224.0)


def forward_matrix(matrix, full_range):
    """M (3,3) fp64: rows Y, Cb, Cr, from RGB levels to YCbCr levels (offsets yo / 128 not included)."""
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    _, ys, cs = scales(full_range)
    return np.array([[kr * ys / 255, kg * ys / 255, kb * ys / 255],
                     [-kr / (2 * (1 - kb)) * cs / 255, -kg / (2 * (1 - kb)) * cs / 255, 0.5 * cs / 255],
                     [0.5 * cs / 255, -kg / (2 * (1 - kr)) * cs / 255, -kb / (2 * (1 - kr)) * cs / 255]], np.float64)


def q_table(matrix, full_range):
    """Q = rint(M * 65536), (3,3) int64."""
    return np.rint(forward_matrix(matrix, full_range) * 65536.0).astype(np.int64)


def frame_bytes(h, w):
    return h * w + 2 * ((h + 1) // 2) * ((w + 1) // 2)


# ---------------------------------------------------------------- output direction: uint8 RGB HWC -> I420, integers
def colours_to_ycc_int(rgb, matrix, full_range):
    """Constant-colour blocks: (..., 3) integer RGB -> (..., 3) Y, Cb, Cr levels by the integer formula.  For a block of
    one colour S = 4 RGB (centre) or 8 RGB (left), and both chroma formulas reduce to the 16-bit shift below."""
    q = q_table(matrix, full_range)
    yo = scales(full_range)[0]
    p = rgb.astype(np.int64)
    y = (p @ q[0] + (yo << 16) + (1 << 15)) >> 16
    cb = (p @ q[1] + (128 << 16) + (1 << 15)) >> 16
    cr = (p @ q[2] + (128 << 16) + (1 << 15)) >> 16
    return np.clip(np.stack([y, cb, cr], -1), 0, 255)


def colours_to_ycc_f64(rgb, matrix, full_range):
    """(..., 3) RGB levels -> (..., 3) exact YCbCr levels in fp64 (not rounded, not clipped)."""
    m = forward_matrix(matrix, full_range)
    return rgb.astype(np.float64) @ m.T + np.array([scales(full_range)[0], 128.0, 128.0])


def rgb_to_yuv420(rgb, matrix, full_range, siting):
    """(n,H,W,3) uint8 -> (n, frame_bytes) uint8, H and W even."""
    n, H, W, _ = rgb.shape
    assert H % 2 == 0 and W % 2 == 0
    q = q_table(matrix, full_range)
    yo = scales(full_range)[0]
    p = rgb.astype(np.int64)
    y = np.clip((p @ q[0] + (yo << 16) + (1 << 15)) >> 16, 0, 255)
    rows = p[:, 0::2] + p[:, 1::2]                                   # (n, H/2, W, 3): rows 2j + 2j+1
    if siting == 'center':
        s = rows[:, :, 0::2] + rows[:, :, 1::2]
        shift = 18
    else:
        left = np.concatenate([rows[:, :, :1], rows[:, :, 1:-1:2]], 2)   # x-1 at x = 2i, clamped to 0
        s = left + 2 * rows[:, :, 0::2] + rows[:, :, 1::2]
        shift = 19
    cb = np.clip((s @ q[1] + (128 << shift) + (1 << (shift - 1))) >> shift, 0, 255)
    cr = np.clip((s @ q[2] + (128 << shift) + (1 << (shift - 1))) >> shift, 0, 255)
    assert max(np.abs(p @ q[0]).max(), np.abs(s @ q[1]).max(), np.abs(s @ q[2]).max()) + (128 << 19) + (1 << 18) < 2 ** 31
    return np.concatenate([y.reshape(n, -1), cb.reshape(n, -1), cr.reshape(n, -1)], 1).astype(np.uint8)


# ---------------------------------------------------------------- input direction: I420 -> RGB in [0,1]
def upsample_taps(n_luma, n_chroma, rule):
    """Along one axis: (idx (n_luma, 2), weight (n_luma, 2)) of the two chroma taps of every luma position, indices
    clamped; the weights of a position sum to 4.  rule 'center': even p -> (p/2 - 1, p/2) x (1, 3), odd p ->
    ((p-1)/2, (p+1)/2) x (3, 1).  rule 'left': even p -> p/2 x 4, odd p -> ((p-1)/2, (p+1)/2) x (2, 2)."""
    p = np.arange(n_luma)
    odd = (p % 2) == 1
    if rule == 'center':
        i0 = np.where(odd, (p - 1) // 2, p // 2 - 1)
        i1 = i0 + 1
        w0 = np.where(odd, 3, 1)
        w1 = 4 - w0
    else:
        i0 = np.where(odd, (p - 1) // 2, p // 2)
        i1 = np.where(odd, (p + 1) // 2, p // 2)
        w0 = np.where(odd, 2, 4)
        w1 = 4 - w0
    idx = np.clip(np.stack([i0, i1], 1), 0, n_chroma - 1)
    return idx, np.stack([w0, w1], 1)


def upsample16(c, h, w, siting):
    """(n, ch, cw) integer chroma plane -> (n, h, w) int64 in sixteenths: rows by the centre rule, columns by the
    siting's rule."""
    ri, rw = upsample_taps(h, c.shape[1], 'center')
    ci, cwt = upsample_taps(w, c.shape[2], siting)
    c = c.astype(np.int64)
    v = c[:, ri[:, 0]] * rw[:, 0, None] + c[:, ri[:, 1]] * rw[:, 1, None]              # (n, h, cw)
    return v[:, :, ci[:, 0]] * cwt[:, 0] + v[:, :, ci[:, 1]] * cwt[:, 1]


def planes(yuv, h, w):
    ch, cw = (h + 1) // 2, (w + 1) // 2
    n = yuv.shape[0]
    return (yuv[:, :h * w].reshape(n, h, w), yuv[:, h * w:h * w + ch * cw].reshape(n, ch, cw),
            yuv[:, h * w + ch * cw:].reshape(n, ch, cw))


def ycc_to_rgb_f64(y, cb16, cr16, matrix, full_range, clamp=True):
    """Y levels and chroma in sixteenths of a level (any broadcastable shapes) -> stacked (3, ...) fp64 RGB in [0,1]."""
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    yo, ys, cs = scales(full_range)
    yn = (np.asarray(y, np.float64) - yo) / ys
    cb = (np.asarray(cb16, np.float64) / 16.0 - 128.0) / cs
    cr = (np.asarray(cr16, np.float64) / 16.0 - 128.0) / cs
    r = yn + 2 * (1 - kr) * cr
    b = yn + 2 * (1 - kb) * cb
    g = yn - (2 * kb * (1 - kb) / kg) * cb - (2 * kr * (1 - kr) / kg) * cr
    out = np.stack(np.broadcast_arrays(r, g, b), 0)
    return np.clip(out, 0.0, 1.0) if clamp else out


def yuv420_to_rgb(yuv, h, w, matrix, full_range, siting):
    """(n, frame_bytes) uint8 -> (n,3,h,w) fp64 in [0,1]."""
    y, u, v = planes(yuv, h, w)
    out = ycc_to_rgb_f64(y, upsample16(u, h, w, siting), upsample16(v, h, w, siting), matrix, full_range)
    return out.transpose(1, 0, 2, 3)
