"""numpy restatement of the two conversions of 10- and 12-bit YUV 4:2:0, shared by
tests/test_yuv_depth_cpu.py and tests/test_hip_yuv_depth.py.  Nothing here imports the package.  The output direction
is the SPECIFICATION: one fp32 step (clamp, times 65535, round half even -- numpy reproduces it bit for bit) and then
exact int64 arithmetic; the GPU must equal rgb_f32_to_yuv420p word for word.  The input direction is stated in fp64.
Depth 8 is defined by the same formulas and is used only to compare with section 7e's (tests/yuv_ref.py)."""
import numpy as np

from tests import yuv_ref as R8

KR_KB = R8.KR_KB
CONFIGS = R8.CONFIGS                             # (matrix, full_range)
SITINGS = R8.SITINGS
DEPTHS = (10, 12)
CASES = [(d, s, m, fr) for d in DEPTHS for s in SITINGS for (m, fr) in CONFIGS]      # 2 depths x 2 sitings x 4 pairs
SHIFT = 24

# Q = rint(M_d * 2^24), rows Y / Cb / Cr (test_yuv_depth_cpu.py recomputes them from Kr and Kb)
TABLES = {
    (10, 'bt601', False): [[67054, 131640, 25566], [-38705, -75985, 114690], [114690, -96038, -18651]],
    (10, 'bt601', True): [[78306, 153731, 29856], [-44191, -86755, 130946], [130946, -109651, -21295]],
    (10, 'bt709', False): [[47678, 160390, 16192], [-26280, -88409, 114690], [114690, -104173, -10516]],
    (10, 'bt709', True): [[55678, 187305, 18909], [-30006, -100940, 130946], [130946, -118939, -12007]],
    (12, 'bt601', False): [[268214, 526561, 102262], [-154818, -303941, 458759], [458759, -384153, -74606]],
    (12, 'bt601', True): [[313452, 615373, 119510], [-176892, -347276, 524168], [524168, -438925, -85243]],
    (12, 'bt709', False): [[190710, 641561, 64766], [-105122, -353637, 458759], [458759, -416693, -42066]],
    (12, 'bt709', True): [[222876, 749770, 75690], [-120110, -404058, 524168], [524168, -476105, -48063]],
}


def scales(depth, full_range):
    """(yo, ys, cs, mid) at `depth` bits."""
    if full_range:
        return 0, float((1 << depth) - 1), float((1 << depth) - 1), 1 << (depth - 1)
    up = depth - 8
    return 16 << up, float(219 << up), float(224 << up), 128 << up


def forward_matrix(depth, matrix, full_range):
    """M_d (3,3) fp64: rows Y, Cb, Cr, from 16-bit RGB codes q in [0, 65535] to YCbCr codes at `depth` bits."""
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    _, ys, cs, _ = scales(depth, full_range)
    return np.array([[kr * ys / 65535, kg * ys / 65535, kb * ys / 65535],
                     [-kr / (2 * (1 - kb)) * cs / 65535, -kg / (2 * (1 - kb)) * cs / 65535, 0.5 * cs / 65535],
                     [0.5 * cs / 65535, -kg / (2 * (1 - kr)) * cs / 65535, -kb / (2 * (1 - kr)) * cs / 65535]], np.float64)


def q_table(depth, matrix, full_range):
    return np.rint(forward_matrix(depth, matrix, full_range) * float(1 << SHIFT)).astype(np.int64)


def frame_samples(h, w):
    return h * w + 2 * ((h + 1) // 2) * ((w + 1) // 2)


def frame_bytes(h, w):
    return 2 * frame_samples(h, w)


# ---------------------------------------------------------------- output direction: fp32 RGB CHW -> I420 at d bits
def quantize16(v):
    """The one float step: float32 array -> int64 codes in [0, 65535].  v < 0 and NaN give 0 (the comparison v > 0 is
    false for both), v > 1 gives 65535; ONE fp32 multiply and one round half even."""
    v = np.asarray(v, np.float32)
    c = np.where(v > np.float32(0), v, np.float32(0)).astype(np.float32)
    c = np.where(c < np.float32(1), c, np.float32(1)).astype(np.float32)
    return np.rint(c * np.float32(65535.0)).astype(np.int64)


def codes_to_ycc_int(q, depth, matrix, full_range):
    """Constant-colour blocks: (..., 3) int64 16-bit codes -> (..., 3) Y, Cb, Cr by the integer formula.  For a block of
    one colour S = 4 q (centre) or 8 q (left), and both chroma formulas reduce to the 24-bit shift below."""
    t = q_table(depth, matrix, full_range)
    yo, _, _, mid = scales(depth, full_range)
    q = q.astype(np.int64)
    half = 1 << (SHIFT - 1)
    y = (q @ t[0] + (yo << SHIFT) + half) >> SHIFT
    cb = (q @ t[1] + (mid << SHIFT) + half) >> SHIFT
    cr = (q @ t[2] + (mid << SHIFT) + half) >> SHIFT
    return np.clip(np.stack([y, cb, cr], -1), 0, (1 << depth) - 1)


def codes_to_ycc_f64(v, depth, matrix, full_range):
    """(..., 3) RGB as 16-bit codes (any real values) -> (..., 3) exact YCbCr codes in fp64, not rounded, not clipped."""
    yo, _, _, mid = scales(depth, full_range)
    return np.asarray(v, np.float64) @ forward_matrix(depth, matrix, full_range).T + np.array([yo, mid, mid], np.float64)


def chroma_sums(q, siting):
    """(n,H,W,3) int64 -> (S (n,H/2,W/2,3), shift): the sum of the 2x2 block (centre, 26) or of (1,2,1) x 2 rows around
    the left column with x-1 clamped to 0 (left, 27)."""
    rows = q[:, 0::2] + q[:, 1::2]
    if siting == 'center':
        return rows[:, :, 0::2] + rows[:, :, 1::2], SHIFT + 2
    left = np.concatenate([rows[:, :, :1], rows[:, :, 1:-1:2]], 2)
    return left + 2 * rows[:, :, 0::2] + rows[:, :, 1::2], SHIFT + 3


def rgb_f32_to_yuv420p(rgb, depth, matrix, full_range, siting):
    """(n,3,H,W) float32 -> (n, frame_samples) uint16, H and W even."""
    n, c, H, W = rgb.shape
    assert c == 3 and H % 2 == 0 and W % 2 == 0 and rgb.dtype == np.float32
    t = q_table(depth, matrix, full_range)
    yo, _, _, mid = scales(depth, full_range)
    top = (1 << depth) - 1
    q = quantize16(rgb).transpose(0, 2, 3, 1)                         # (n,H,W,3) int64
    y = np.clip((q @ t[0] + (yo << SHIFT) + (1 << (SHIFT - 1))) >> SHIFT, 0, top)
    s, shift = chroma_sums(q, siting)
    cb = np.clip((s @ t[1] + (mid << shift) + (1 << (shift - 1))) >> shift, 0, top)
    cr = np.clip((s @ t[2] + (mid << shift) + (1 << (shift - 1))) >> shift, 0, top)
    return np.concatenate([y.reshape(n, -1), cb.reshape(n, -1), cr.reshape(n, -1)], 1).astype(np.uint16)


# ---------------------------------------------------------------- input direction: I420 at d bits -> RGB in [0,1], fp64
def planes(yuv, h, w):
    return R8.planes(yuv, h, w)


def ycc_to_rgb_f64(y, cb16, cr16, depth, matrix, full_range, clamp=True):
    """Y codes and chroma in sixteenths of a code -> stacked (3, ...) fp64 RGB in [0,1]."""
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    yo, ys, cs, mid = scales(depth, full_range)
    yn = (np.asarray(y, np.float64) - yo) / ys
    cb = (np.asarray(cb16, np.float64) / 16.0 - mid) / cs
    cr = (np.asarray(cr16, np.float64) / 16.0 - mid) / cs
    r = yn + 2 * (1 - kr) * cr
    b = yn + 2 * (1 - kb) * cb
    g = yn - (2 * kb * (1 - kb) / kg) * cb - (2 * kr * (1 - kr) / kg) * cr
    out = np.stack(np.broadcast_arrays(r, g, b), 0)
    return np.clip(out, 0.0, 1.0) if clamp else out


def yuv420p_to_rgb(yuv, h, w, depth, matrix, full_range, siting):
    """(n, frame_samples) uint16 -> (n,3,h,w) fp64 in [0,1]; a sample above 2^depth - 1 is read as 2^depth - 1."""
    yuv = np.minimum(yuv.astype(np.int64), (1 << depth) - 1)
    y, u, v = planes(yuv, h, w)
    out = ycc_to_rgb_f64(y, R8.upsample16(u, h, w, siting), R8.upsample16(v, h, w, siting), depth, matrix, full_range)
    return out.transpose(1, 0, 2, 3)
