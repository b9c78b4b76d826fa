"""Specification of the tOF metric's optical flow: dense Farneback flow with the one parameter set both reference
call sites use (pyr_scale 0.5, levels 3, winsize 15, iterations 3, poly_n 5, poly_sigma 1.2, flags 0), in numpy.

Written from the published algorithm (G. Farneback, "Two-frame motion estimation based on polynomial expansion",
SCIA 2003) and the widely known structure of OpenCV's implementation.  It has NOT been compared with OpenCV: no
machine of this project has cv2.  DESIGN.md section 7f is the text this file follows.

Every function takes the number format: dt = np.float64 is the specification, dt = np.float32 (`alt32`) does every
sum and product of image data in true float32, tap by tap on float32 arrays, in the order the HIP kernels use.
Constants (filter taps, the inverse Gram matrix, sampling positions) are always computed in fp64 and then rounded
to dt, as the kernels' host side does.

Flow layout: (h, w, 2) float, channel 0 = x (along W), channel 1 = y, from `prev` to `next`."""
import numpy as np

POLY_N, POLY_SIGMA, WINSIZE, ITERS, MAX_LEVEL, MIN_SIZE = 5, 1.2, 15, 3, 3, 32
BORDER = (0.14, 0.14, 0.4472, 0.4472, 0.4472)
KEYS_OFFICIAL = ('PSNR', 'SSIM', 'LPIPS', 'tOF', 'tLP100')


# ---- geometry ------------------------------------------------------------------------------------------------
def gray_u8(rgb):
    """uint8 gray of uint8 RGB: (4899 R + 9617 G + 1868 B + 8192) >> 14."""
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    return ((4899 * r + 9617 * g + 1868 * b + 8192) >> 14).astype(np.uint8)


def top_level(h, w):
    """L: the largest k <= 3 with min(w, h) * 0.5^j >= 32 for every j in 1..k."""
    k = 0
    while k < MAX_LEVEL and min(h, w) * 0.5 ** (k + 1) >= MIN_SIZE:
        k += 1
    return k


def level_size(h, w, k):
    """(rint(h s), rint(w s)), s = 0.5^k, round half to even."""
    s = 0.5 ** k
    return int(np.rint(h * s)), int(np.rint(w * s))


def blur_taps(k):
    """Gaussian of the level image: sigma = (1/s - 1)/2, size max(rint(5 sigma) | 1, 3); [1/4, 1/2, 1/4] at k = 0."""
    sigma = (2.0 ** k - 1.0) * 0.5
    size = max(int(np.rint(5.0 * sigma)) | 1, 3)
    if sigma == 0.0:
        return np.array([0.25, 0.5, 0.25])
    x = np.arange(size, dtype=np.float64) - size // 2
    t = np.exp(-x * x / (2.0 * sigma * sigma))
    return t / t.sum()


def poly_constants():
    """g, xg, xxg on -5..5 and (ig11, ig03, ig33, ig55) of the inverse Gram matrix, fp64."""
    x = np.arange(-POLY_N, POLY_N + 1, dtype=np.float64)
    g = np.exp(-x * x / (2.0 * POLY_SIGMA * POLY_SIGMA))
    g /= g.sum()
    gg = g[:, None] * g[None, :]
    X, Y = x[None, :], x[:, None]
    G00, G11, G33, G55 = gg.sum(), (gg * X * X).sum(), (gg * X ** 4).sum(), (gg * X * X * Y * Y).sum()
    G = np.zeros((6, 6))
    G[0, 0] = G00
    G[1, 1] = G[2, 2] = G[0, 3] = G[0, 4] = G[3, 0] = G[4, 0] = G11
    G[3, 3] = G[4, 4] = G33
    G[3, 4] = G[4, 3] = G[5, 5] = G55
    inv = np.linalg.inv(G)
    return g, x * g, x * x * g, (inv[1, 1], inv[0, 3], inv[3, 3], inv[5, 5])


def _src(n_dst, n_src):
    """Bilinear source taps of one axis: src = (dst + 0.5) (n_src / n_dst) - 0.5; (i0, i1, frac) with the
    neighbours clamped to the image.  fp64."""
    s = (np.arange(n_dst, dtype=np.float64) + 0.5) * (n_src / n_dst) - 0.5
    i0 = np.floor(s)
    f = s - i0
    i0 = i0.astype(np.int64)
    return np.clip(i0, 0, n_src - 1), np.clip(i0 + 1, 0, n_src - 1), f


# ---- linear stages -------------------------------------------------------------------------------------------
def _shift(p, k, n, axis):
    return p[k:k + n] if axis == 0 else p[:, k:k + n]


def blur_full(gray, k, dt):
    """Separable Gaussian of the full-resolution frame, reflect-101 borders, rows (along W) first."""
    taps = blur_taps(k).astype(dt)
    r = len(taps) // 2
    img = gray.astype(dt)
    for axis in (1, 0):
        pad = np.pad(img, [(r, r) if a == axis else (0, 0) for a in (0, 1)], mode='reflect')
        n = img.shape[axis]
        acc = taps[0] * _shift(pad, 0, n, axis)
        for i in range(1, len(taps)):
            acc = acc + taps[i] * _shift(pad, i, n, axis)
        img = acc
    return img


def resize_bilinear(img, oh, ow, dt):
    """img (h, w[, c]) -> (oh, ow[, c]): along W first (top and bottom rows), then along H."""
    y0, y1, fy = _src(oh, img.shape[0])
    x0, x1, fx = _src(ow, img.shape[1])
    fx, fy = fx.astype(dt), fy.astype(dt)
    if img.ndim == 3:
        fx, fy = fx[None, :, None], fy[:, None, None]
    else:
        fx, fy = fx[None, :], fy[:, None]
    one = dt(1)
    top = img[y0][:, x0] * (one - fx) + img[y0][:, x1] * fx
    bot = img[y1][:, x0] * (one - fx) + img[y1][:, x1] * fx
    return top * (one - fy) + bot * fy


def level_image(gray, k, dt=np.float64):
    h, w = gray.shape
    lh, lw = level_size(h, w, k)
    return resize_bilinear(blur_full(gray, k, dt), lh, lw, dt)


def polyexp(img, dt=np.float64):
    """(h, w) -> (5, h, w): (r_y, r_x, r_yy, r_xx, r_xy).  Replicate borders, vertical pass then horizontal; the
    symmetric taps are paired as (I[+k] + I[-k]) t[k] and the antisymmetric ones as (I[+k] - I[-k]) t[k]."""
    g, xg, xxg, inv = poly_constants()
    n = POLY_N
    g, xg, xxg = g[n:].astype(dt), xg[n:].astype(dt), xxg[n:].astype(dt)      # taps 0..5
    ig11, ig03, ig33, ig55 = (dt(v) for v in inv)

    def passes(a, axis):
        pad = np.pad(a, [(n, n) if ax == axis else (0, 0) for ax in (0, 1)], mode='edge')
        m = a.shape[axis]
        s0 = g[0] * _shift(pad, n, m, axis)
        s1 = s2 = None
        for k in range(1, n + 1):
            p, q = _shift(pad, n + k, m, axis), _shift(pad, n - k, m, axis)
            s0 = s0 + g[k] * (p + q)
            s1 = xg[k] * (p - q) if s1 is None else s1 + xg[k] * (p - q)
            s2 = xxg[k] * (p + q) if s2 is None else s2 + xxg[k] * (p + q)
        return s0, s1, s2

    img = img.astype(dt)
    row0, row1, row2 = passes(img, 0)            # g, xg, xxg along y
    b1, b2, b4 = passes(row0, 1)
    b3, b5, _ = passes(row1, 1)
    b6, _, _ = passes(row2, 1)
    return np.stack([b3 * ig11, b2 * ig11, b1 * ig03 + b6 * ig33, b1 * ig03 + b4 * ig33, b5 * ig55])


def box_mean(M, dt=np.float64):
    """(5, h, w): 15 x 15 box sum with replicate borders (along W first, left to right; then along H), times 1/225."""
    r = WINSIZE // 2
    out = M.astype(dt)
    for axis in (2, 1):
        pad = np.pad(out, [(r, r) if a == axis else (0, 0) for a in (0, 1, 2)], mode='edge')
        n = out.shape[axis]
        sl = (lambda k: pad[:, :, k:k + n]) if axis == 2 else (lambda k: pad[:, k:k + n])
        acc = sl(0)
        for k in range(1, WINSIZE):
            acc = acc + sl(k)
        out = acc
    return out * dt(1.0 / (WINSIZE * WINSIZE))


# ---- the non-linear stages -----------------------------------------------------------------------------------
def update_matrices(R0, R1, flow, dt=np.float64):
    """Step 6: (5, h, w) expansions of both frames and the current flow (h, w, 2) -> M (5, h, w)."""
    _, h, w = R0.shape
    R0, R1, flow = R0.astype(dt), R1.astype(dt), flow.astype(dt)
    dx, dy = flow[..., 0], flow[..., 1]
    ys, xs = np.mgrid[0:h, 0:w]
    fx, fy = xs.astype(dt) + dx, ys.astype(dt) + dy
    inside = (fx >= 0) & (fx < w - 1) & (fy >= 0) & (fy < h - 1)       # 0 <= floor(fx) < w - 1, NaN is outside
    x1 = np.floor(np.where(inside, fx, dt(0))).astype(np.int64)
    y1 = np.floor(np.where(inside, fy, dt(0))).astype(np.int64)
    x1, y1 = np.minimum(x1, w - 2), np.minimum(y1, h - 2)              # only touched where outside
    ax, ay = (fx - x1.astype(dt)), (fy - y1.astype(dt))
    one = dt(1)
    a00, a01, a10, a11 = (one - ax) * (one - ay), ax * (one - ay), (one - ax) * ay, ax * ay
    S = a00 * R1[:, y1, x1] + a01 * R1[:, y1, x1 + 1] + a10 * R1[:, y1 + 1, x1] + a11 * R1[:, y1 + 1, x1 + 1]
    half, quarter = dt(0.5), dt(0.25)
    r2 = np.where(inside, (R0[0] - S[0]) * half, dt(0))
    r3 = np.where(inside, (R0[1] - S[1]) * half, dt(0))
    r4 = np.where(inside, (R0[2] + S[2]) * half, R0[2])
    r5 = np.where(inside, (R0[3] + S[3]) * half, R0[3])
    r6 = np.where(inside, (R0[4] + S[4]) * quarter, R0[4] * half)
    r2 = r2 + (r4 * dy + r6 * dx)
    r3 = r3 + (r6 * dy + r5 * dx)
    scale = np.ones((h, w), dt)
    bd = [dt(v) for v in BORDER]
    for d in range(5):                                                  # left, right, top, bottom: in this order
        scale[:, d] = scale[:, d] * bd[d]
    for d in range(5):
        scale[:, w - 1 - d] = scale[:, w - 1 - d] * bd[d]
    for d in range(5):
        scale[d, :] = scale[d, :] * bd[d]
    for d in range(5):
        scale[h - 1 - d, :] = scale[h - 1 - d, :] * bd[d]
    r2, r3, r4, r5, r6 = (r * scale for r in (r2, r3, r4, r5, r6))
    return np.stack([r4 * r4 + r6 * r6, (r4 + r5) * r6, r5 * r5 + r6 * r6, r4 * r2 + r6 * r3, r6 * r2 + r5 * r3])


def solve(B, dt=np.float64):
    g11, g12, g22, h1, h2 = B.astype(dt)
    idet = dt(1) / ((g11 * g22 - g12 * g12) + dt(1e-3))
    return np.stack([(g11 * h2 - g12 * h1) * idet, (g22 * h1 - g12 * h2) * idet], axis=-1)


def blur_solve(M, dt=np.float64):
    return solve(box_mean(M, dt), dt)


def resize_flow(flow, oh, ow, dt=np.float64):
    return resize_bilinear(flow.astype(dt), oh, ow, dt) * dt(2)


# ---- the whole flow ------------------------------------------------------------------------------------------
def farneback(prev_gray, next_gray, dt=np.float64, trace=None):
    """uint8 gray frames (h, w) -> flow (h, w, 2) in dt.  trace: a dict that receives the per-level stage data."""
    h, w = prev_gray.shape
    flow = None
    for k in range(top_level(h, w), -1, -1):
        lh, lw = level_size(h, w, k)
        flow = np.zeros((lh, lw, 2), dt) if flow is None else resize_flow(flow, lh, lw, dt)
        R0, R1 = polyexp(level_image(prev_gray, k, dt), dt), polyexp(level_image(next_gray, k, dt), dt)
        M = update_matrices(R0, R1, flow, dt)
        for it in range(ITERS):
            flow = blur_solve(M, dt)
            if it < ITERS - 1:
                M = update_matrices(R0, R1, flow, dt)
        if trace is not None:
            trace[k] = dict(R0=R0, R1=R1, M=M, flow=flow)
    return flow


def alt32(prev_gray, next_gray):
    return farneback(prev_gray, next_gray, np.float32)


def flows_of_sequence(seq_u8, h=None, w=None, dt=np.float64):
    """(t, fh, fw, 3) uint8 RGB -> (t - 1, h, w, 2) flows of consecutive frames on the top-left h x w."""
    h, w = h or seq_u8.shape[1], w or seq_u8.shape[2]
    gray = [gray_u8(f[:h, :w]) for f in seq_u8]
    return np.stack([farneback(gray[i], gray[i + 1], dt) for i in range(len(gray) - 1)])


def epe_mean(flow_a, flow_b, window=None):
    """mean(sqrt(dx^2 + dy^2)) of float32 flows: the per-pixel value in float32, the mean in fp64."""
    a, b = np.asarray(flow_a, np.float32), np.asarray(flow_b, np.float32)
    if window is not None:
        y, x, ch, cw = window
        a, b = a[..., y:y + ch, x:x + cw, :], b[..., y:y + ch, x:x + cw, :]
    d = a - b
    e = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1])
    return e.astype(np.float64).mean(axis=(-2, -1))


def crop_8x8_window(h, w):
    ch, cw = (h // 32) * 32, (w // 32) * 32
    while ch > h - 16:
        ch -= 32
    while cw > w - 16:
        cw -= 32
    return (h - ch) // 2, (w - cw) // 2, ch, cw


def tof(true_seq, pred_seq, official=True, dt=np.float64):
    """Per-pair tOF of two uint8 sequences that are already the evaluated range: flows on the size-matched
    (top-left cropped) frames; the official protocol then applies crop_8x8 to the flows, the in-loop metric
    takes the whole frame."""
    h, w = min(true_seq.shape[1], pred_seq.shape[1]), min(true_seq.shape[2], pred_seq.shape[2])
    ft = flows_of_sequence(true_seq, h, w, dt).astype(np.float32)
    fp = flows_of_sequence(pred_seq, h, w, dt).astype(np.float32)
    return epe_mean(ft, fp, crop_8x8_window(h, w) if official else None)
