"""numpy specification of the three planar conversions: 4:2:0, 4:2:2 and 4:4:4 at 8, 10 and 12
bits with any (Kr, Kb), shared by tests/test_yuv_planar_cpu.py and tests/test_hip_yuv_planar.py.  Nothing here imports
the package.  It builds on tests/yuv_ref.py and tests/yuv_depth_ref.py where they coincide (upsample_taps per axis,
quantize16, the fp64 matrices' shape) and computes every table from (Kr, Kb).  The output direction is the
SPECIFICATION in exact integers (the GPU's bytes and words must be equal); the input direction is stated in fp64."""
import numpy as np

from tests import yuv_depth_ref as RD
from tests import yuv_ref as R8

KR_KB = dict(R8.KR_KB, bt2020=(0.2627, 0.0593))  # BT.2020 non-constant luminance
MATRICES = ('bt601', 'bt709', 'bt2020')
CONFIGS = [(m, fr) for m in MATRICES for fr in (False, True)]
SITINGS = R8.SITINGS
CHROMAS = ('420', '422', '444')
SUB = {'420': (2, 2), '422': (2, 1), '444': (1, 1)}      # (sx, sy)
DEPTHS = (8, 10, 12)

# rint(M * 2^16) (depth 8) and rint(M_d * 2^24) (10, 12) for BT.2020, rows Y / Cb / Cr: the tables printed in DESIGN.md
# section 7l (test_yuv_planar_cpu.py recomputes them from Kr and Kb)
BT2020_TABLES = {
    (8, False): [[14786, 38160, 3338], [-8038, -20746, 28784], [28784, -26469, -2315]],
    (8, True): [[17216, 44433, 3886], [-9151, -23617, 32768], [32768, -30133, -2635]],
    (10, False): [[58913, 152048, 13299], [-32028, -82661, 114690], [114690, -105465, -9224]],
    (10, True): [[68799, 177563, 15530], [-36568, -94378, 130946], [130946, -120414, -10532]],
    (12, False): [[235652, 608192, 53194], [-128113, -330646, 458759], [458759, -421862, -36897]],
    (12, True): [[275398, 710772, 62166], [-146379, -377789, 524168], [524168, -482010, -42158]],
}


def scales(depth, full_range):
    """(yo, ys, cs, mid) at `depth` bits; depth 8 gives yuv_ref.scales and the mid value 128."""
    return RD.scales(depth, full_range)


def shift_of(depth):
    return 16 if depth == 8 else RD.SHIFT


def forward_matrix(depth, matrix, full_range):
    """M (3,3) fp64, rows Y, Cb, Cr: from RGB levels 0..255 (depth 8) or 16-bit codes 0..65535 (10, 12) to YCbCr codes
    at `depth` bits, offsets not included.  The expressions are yuv_ref.forward_matrix's, with (Kr, Kb) from KR_KB."""
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    _, ys, cs, _ = scales(depth, full_range)
    i = 255 if depth == 8 else 65535
    return np.array([[kr * ys / i, kg * ys / i, kb * ys / i],
                     [-kr / (2 * (1 - kb)) * cs / i, -kg / (2 * (1 - kb)) * cs / i, 0.5 * cs / i],
                     [0.5 * cs / i, -kg / (2 * (1 - kr)) * cs / i, -kb / (2 * (1 - kr)) * cs / i]], np.float64)


def q_table(depth, matrix, full_range):
    """rint(M * 2^16) at depth 8, rint(M_d * 2^24) above; (3,3) int64."""
    return np.rint(forward_matrix(depth, matrix, full_range) * float(1 << shift_of(depth))).astype(np.int64)


def chroma_size(h, w, chroma):
    sx, sy = SUB[chroma]
    return (h + sy - 1) // sy, (w + sx - 1) // sx


def frame_samples(h, w, chroma):
    ch, cw = chroma_size(h, w, chroma)
    return h * w + 2 * ch * cw


def frame_bytes(h, w, chroma, depth=8):
    return frame_samples(h, w, chroma) * (2 if depth > 8 else 1)


def planes(yuv, h, w, chroma):
    """(n, frame_samples) -> Y (n,h,w), U and V (n,ch,cw) views."""
    ch, cw = chroma_size(h, w, chroma)
    n = yuv.shape[0]
    return (yuv[:, :h * w].reshape(n, h, w), yuv[:, h * w:h * w + ch * cw].reshape(n, ch, cw),
            yuv[:, h * w + ch * cw:].reshape(n, ch, cw))


# ---------------------------------------------------------------- output direction: integers
def chroma_sums(p, chroma, siting):
    """(n,H,W,3) int64 -> (S (n,ch,cw,3), t): the tap-weighted sum of every chroma sample and log2 of the total weight.
    Vertically a sub-sampled axis adds rows 2j and 2j+1; horizontally 'center' adds the pair, 'left' takes (1,2,1)
    over x-1, x, x+1 at x = 2i with x-1 clamped to 0; an axis that is not sub-sampled takes the pixel."""
    sx, sy = SUB[chroma]
    t = 0
    if sy == 2:
        p, t = p[:, 0::2] + p[:, 1::2], t + 1
    if sx == 2 and siting == 'center':
        p, t = p[:, :, 0::2] + p[:, :, 1::2], t + 1
    elif sx == 2:
        left = np.concatenate([p[:, :, :1], p[:, :, 1:-1:2]], 2)
        p, t = left + 2 * p[:, :, 0::2] + p[:, :, 1::2], t + 2
    return p, t


def check_out_shape(H, W, chroma):
    sx, sy = SUB[chroma]
    assert H % sy == 0 and W % sx == 0, (H, W, chroma)


def ints_to_yuv(p, chroma, depth, matrix, full_range, siting):
    """(n,H,W,3) int64 RGB (levels at depth 8, 16-bit codes above) -> (n, frame_samples) int64 YUV codes."""
    n, H, W, _ = p.shape
    check_out_shape(H, W, chroma)
    q, sh = q_table(depth, matrix, full_range), shift_of(depth)
    yo, _, _, mid = scales(depth, full_range)
    top = (1 << depth) - 1
    y = np.clip((p @ q[0] + (yo << sh) + (1 << (sh - 1))) >> sh, 0, top)
    s, t = chroma_sums(p, chroma, siting)
    sh += t
    cb = np.clip((s @ q[1] + (mid << sh) + (1 << (sh - 1))) >> sh, 0, top)
    cr = np.clip((s @ q[2] + (mid << sh) + (1 << (sh - 1))) >> sh, 0, top)
    if depth == 8:                                   # the device accumulates in 32 bits there
        assert max(np.abs(p @ q[0]).max(), np.abs(s @ q[1]).max(), np.abs(s @ q[2]).max()) + (mid << sh) + (1 << sh) < 2 ** 31
    return np.concatenate([y.reshape(n, -1), cb.reshape(n, -1), cr.reshape(n, -1)], 1)


def rgb_u8_to_yuv(rgb, chroma, matrix, full_range, siting):
    """(n,H,W,3) uint8 -> (n, frame_bytes) uint8: tg_rgb_u8_to_yuv_planar."""
    assert rgb.dtype == np.uint8
    return ints_to_yuv(rgb.astype(np.int64), chroma, 8, matrix, full_range, siting).astype(np.uint8)


def rgb_f32_to_yuv(rgb, chroma, depth, matrix, full_range, siting):
    """(n,3,H,W) float32 -> (n, frame_samples) uint16 at depth 10 | 12: tg_rgb_f32_to_yuv_planar16."""
    assert rgb.dtype == np.float32 and rgb.shape[1] == 3 and depth in (10, 12)
    q = RD.quantize16(rgb).transpose(0, 2, 3, 1)
    return ints_to_yuv(q, chroma, depth, matrix, full_range, siting).astype(np.uint16)


def colours_to_ycc_f64(v, depth, matrix, full_range):
    """(..., 3) RGB (levels at depth 8, 16-bit codes above; any real values) -> (..., 3) exact YCbCr codes in fp64,
    not rounded, not clipped."""
    yo, _, _, mid = scales(depth, full_range)
    return np.asarray(v, np.float64) @ forward_matrix(depth, matrix, full_range).T + np.array([yo, mid, mid], np.float64)


def ints_to_yuv_f64(p, chroma, depth, matrix, full_range, siting):
    """The fp64 route of ints_to_yuv: colours_to_ycc_f64 on the pixel (Y) and on the exact tap average (chroma), rounded
    half up and clipped; (n, frame_samples) int64."""
    n = p.shape[0]
    top = (1 << depth) - 1
    s, t = chroma_sums(p, chroma, siting)
    y = colours_to_ycc_f64(p, depth, matrix, full_range)[..., 0]
    c = colours_to_ycc_f64(s.astype(np.float64) / (1 << t), depth, matrix, full_range)
    out = np.concatenate([y.reshape(n, -1), c[..., 1].reshape(n, -1), c[..., 2].reshape(n, -1)], 1)
    return np.clip(np.floor(out + 0.5), 0, top).astype(np.int64)


# ---------------------------------------------------------------- input direction: fp64
def axis_taps(n_luma, n_chroma, sub, rule):
    """yuv_ref.upsample_taps along a sub-sampled axis; along one that is not, the sample itself times 4."""
    if sub == 2:
        return R8.upsample_taps(n_luma, n_chroma, rule)
    p = np.arange(n_luma)
    return np.stack([p, p], 1), np.stack([np.full(n_luma, 4), np.zeros(n_luma, np.int64)], 1)


def upsample16(c, h, w, chroma, siting):
    """(n, ch, cw) integer chroma plane -> (n, h, w) int64 in sixteenths."""
    sx, sy = SUB[chroma]
    ri, rw = axis_taps(h, c.shape[1], sy, 'center')
    ci, cwt = axis_taps(w, c.shape[2], sx, siting)
    c = c.astype(np.int64)
    v = c[:, ri[:, 0]] * rw[:, 0, None] + c[:, ri[:, 1]] * rw[:, 1, None]
    return v[:, :, ci[:, 0]] * cwt[:, 0] + v[:, :, ci[:, 1]] * cwt[:, 1]


def ycc_to_rgb_f64(y, cb16, cr16, depth, matrix, full_range, clamp=True):
    """yuv_depth_ref.ycc_to_rgb_f64 with (Kr, Kb) from KR_KB."""
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


def yuv_to_rgb(yuv, h, w, chroma, depth, matrix, full_range, siting):
    """(n, frame_samples) uint8 / uint16 -> (n,3,h,w) fp64 in [0,1]: tg_yuv_planar_to_rgb_f32 in fp64.  A sample above
    2^depth - 1 is read as 2^depth - 1."""
    yuv = np.minimum(yuv.astype(np.int64), (1 << depth) - 1)
    y, u, v = planes(yuv, h, w, chroma)
    out = ycc_to_rgb_f64(y, upsample16(u, h, w, chroma, siting), upsample16(v, h, w, chroma, siting), depth, matrix,
                         full_range)
    return out.transpose(1, 0, 2, 3)
