"""fp64 references, exact-sum inputs and rounding bounds shared by tests/test_train_reductions_cpu.py
(which checks this module against torch's own double-precision ops) and tests/test_hip_train_reductions.py
(which holds the kernels of csrc/tg_train.hip to it).  Everything here runs on the CPU in float64."""
import math

import numpy as np
import torch

U = 2.0 ** -24                      # unit roundoff of fp32 (round to nearest)


def gamma_k(k):
    """Higham's gamma_k = k u / (1 - k u): a chain of k fp32 additions of terms t_i ends within gamma_k * sum |t_i|."""
    return k * U / (1.0 - k * U)


def exact_values(seed, shape, denom=8, kmax=8):
    """fp32 tensor of values j / denom, integer |j| <= kmax.  Every partial sum of m of them is a multiple of
    1 / denom of magnitude <= m * kmax / denom: exactly representable while m * kmax < 2^24, so ANY summation
    order gives the exact sum (tests assert the size condition where they use it)."""
    j = np.random.RandomState(seed).randint(-kmax, kmax + 1, size=shape)
    return torch.from_numpy((j / float(denom)).astype(np.float32))


def ulp_distance(a, b):
    """|a - b| in units of the fp32 spacing at b (element-wise, float64 result)."""
    a = np.asarray(a, np.float32); b = np.asarray(b, np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.abs(b)).astype(np.float64)


# ---- BatchNorm2d (train) + LeakyReLU ----------------------------------------------------------
def bn_fwd_ref(x, gamma, beta, eps=1e-5, slope=0.2):
    """x (n,c,h,w); returns float64 (y, mean, var_biased, invstd)."""
    x = x.double(); g = gamma.double().view(1, -1, 1, 1); b = beta.double().view(1, -1, 1, 1)
    mean = x.mean((0, 2, 3))
    var = ((x - mean.view(1, -1, 1, 1)) ** 2).mean((0, 2, 3))
    invstd = 1.0 / torch.sqrt(var + eps)
    v = (x - mean.view(1, -1, 1, 1)) * invstd.view(1, -1, 1, 1) * g + b
    return torch.where(v >= 0, v, v * slope), mean, var, invstd


def bn_running_ref(run_mean0, run_var0, mean, var, count, momentum):
    """momentum: the fp32 value the kernel receives; (1 - momentum) is formed in fp32 there (one rounding, counted
    in the test's bound), here in float64."""
    m = float(np.float32(momentum))
    return ((1.0 - m) * run_mean0.double() + m * mean,
            (1.0 - m) * run_var0.double() + m * var * (count / (count - 1.0)))


def bn_bwd_ref(x, y, dy, gamma, mean, invstd, slope=0.2, count=None):
    """Backward of BN(train)+LeakyReLU as a function of the op's own inputs: the mask comes from the forward
    OUTPUT y (y > 0), mean / invstd are the saved statistics.  Returns float64 (dx, dgamma, dbeta, dz, xhat);
    `count`: the global element count when x is one part of a larger batch (dx then needs the global sums:
    see bn_bwd_dx_ref)."""
    x = x.double(); dy = dy.double()
    mu = mean.double().view(1, -1, 1, 1); is_ = invstd.double().view(1, -1, 1, 1)
    dz = torch.where(y.double() > 0, dy, dy * slope)
    xhat = (x - mu) * is_
    dbeta = dz.sum((0, 2, 3)); dgamma = (dz * xhat).sum((0, 2, 3))
    cnt = float(count if count is not None else x.numel() // x.shape[1])
    dx = bn_bwd_dx_ref(dz, xhat, gamma, invstd, dbeta, dgamma, cnt)
    return dx, dgamma, dbeta, dz, xhat


def bn_bwd_dx_ref(dz, xhat, gamma, invstd, sum_dz, sum_dz_xhat, count):
    gs = (gamma.double() * invstd.double()).view(1, -1, 1, 1)
    return gs * (dz - sum_dz.view(1, -1, 1, 1) / count - xhat * sum_dz_xhat.view(1, -1, 1, 1) / count)


def bn_sweep_chain(n_images, hw, threads, vec):
    """Additions one thread of bn_sweep performs: the 16-byte form walks hw / 4 groups with stride `threads`
    (4 elements each), the scalar form hw elements."""
    per_plane = 4 * math.ceil((hw // 4) / threads) if vec else math.ceil(hw / threads)
    return n_images * per_plane


def block_chain(per_thread, threads):
    """Longest chain of additions of a block reduction: the thread's own elements, 6 wave shuffles, one add per wave."""
    return per_thread + 6 + threads // 64


# ---- losses ------------------------------------------------------------------------------------
def charbonnier_ref(x, y, eps=1e-6):
    """Returns (terms r_i = sqrt(d^2 + eps), d / r_i) in float64 with d = x - y exact (the kernel's fp32
    subtraction is one rounding, counted in the test's bound)."""
    d = x.double() - y.double()
    r = torch.sqrt(d * d + eps)
    return r, d / r


def pixel_ref(x, y, mode):
    d = x.double() - y.double()
    if mode == 1:
        return d.abs(), torch.sign(d)
    return d * d, 2.0 * d


def bce_ref(x, target, lsgan=False):
    """Per-element (loss term, x, log(sigmoid(x) + 1e-8), d loss / dx) in float64; 1e-8 is the fp32 constant."""
    x = x.double()
    sig = 1.0 / (1.0 + torch.exp(-x))
    e8 = float(np.float32(1e-8))
    if lsgan:
        t0 = (x - target) ** 2
        g = 2.0 * (x - target)
    else:
        t0 = torch.clamp(x, min=0) - x * target + torch.log1p(torch.exp(-x.abs()))
        g = sig - target
    return t0, x, torch.log(sig + e8), g


def cosine_ref(a, b, eps=1e-8):
    """CosineSimilarityLoss over dim 1 of (n,c,h,w): per-pixel 1 - cos and d(sum (1 - cos)) / da, float64, with
    x / max(|x|, eps) and no gradient through a clamped norm (what autograd of clamp_min gives)."""
    a = a.double(); b = b.double()
    na = a.norm(dim=1, keepdim=True); nb = b.norm(dim=1, keepdim=True)
    nac = na.clamp_min(eps); nbc = nb.clamp_min(eps)
    cs = (a * b).sum(1, keepdim=True) / (nac * nbc)
    k = torch.where(na > eps, cs / (nac * nac), torch.zeros_like(cs))
    return (1.0 - cs).squeeze(1), -(b / (nac * nbc) - k * a)


def adam_ref(p, g, m, v, lr, b1, b2, eps, wd, step):
    """torch.optim.Adam (L2 weight decay) in float64 from fp32 hyper-parameters."""
    f = lambda s: float(np.float32(s))
    lr, b1, b2, eps, wd = f(lr), f(b1), f(b2), f(eps), f(wd)
    p = p.double(); g = g.double() + wd * p
    m = b1 * m.double() + (1 - b1) * g
    v = b2 * v.double() + (1 - b2) * g * g
    bc1 = 1 - b1 ** step; bc2 = 1 - b2 ** step
    return p - (lr / bc1) * m / (torch.sqrt(v) / math.sqrt(bc2) + eps), m, v


# ---- fp32 summation orders (the CPU test shows exact-sum inputs do not care) --------------------
def sum_f32_strided(v, threads, chunks=1):
    """The kernels' order in fp32: `chunks` equal slices; in each, thread t adds elements t, t + threads, ...
    sequentially, 64-lane xor-shuffle trees, waves added in order; slices added in order."""
    v = np.asarray(v, np.float32)
    total = np.float32(0)
    for part in np.array_split(v, chunks):
        pad = (-len(part)) % threads
        rows = np.concatenate([part, np.zeros(pad, np.float32)]).reshape(-1, threads)
        acc = np.zeros(threads, np.float32)
        for r in rows:
            acc = acc + r                                   # float32 + float32 -> float32
        w = acc.reshape(-1, 64)
        o = 32
        while o:
            w = w + w[:, np.arange(64) ^ o]
            o >>= 1
        s = np.float32(0)
        for i in range(w.shape[0]):
            s = np.float32(s + w[i, 0])
        total = np.float32(total + s)
    return total


def sum_f32_pairwise(v):
    v = np.asarray(v, np.float32)
    while len(v) > 1:
        if len(v) & 1:
            v = np.concatenate([v, np.zeros(1, np.float32)])
        v = v[0::2] + v[1::2]
    return np.float32(v[0])


def sum_f32_sequential(v):
    s = np.float32(0)
    for e in np.asarray(v, np.float32):
        s = np.float32(s + e)
    return s


# ---- the BatchNorm shape table: (n, c, h, w) -> (threads, slices, 16-byte form) each row must select ----
BN_CASES = [
    ((3, 3, 4, 8), (256, 1, True)),          # 16-byte, tail only, plane smaller than the block
    ((4, 5, 4, 8), (256, 1, True)),          # one four-image group, no tail
    ((7, 3, 48, 40), (256, 1, True)),        # group + 3-image tail, two strides per plane
    ((5, 3, 64, 128), (1024, 1, True)),      # 1024 threads, group + tail
    ((5, 2, 91, 91), (1024, 1, False)),      # 1024 threads, scalar form
    ((2, 3, 128, 256), (1024, 2, True)),     # 2 slices of 1 image
    ((10, 3, 64, 128), (1024, 2, True)),     # 2 slices of 5 images: group + tail at a non-zero slice base
    ((8, 3, 128, 256), (1024, 8, True)),     # 8 slices
    ((6, 2, 181, 182), (1024, 6, False)),    # 6 slices, scalar form
    ((8, 24, 128, 256), (1024, 8, True)),    # apply kernels past the grid cap
]
GRID_CAP_THREADS = 4096 * 256                # grid_for(): at most 4096 blocks of 256 threads


def bn_geometry(lib, n, c, hw):
    """(threads, slices) from tg_bn_launch_geometry (host only)."""
    import ctypes
    t, s = ctypes.c_int(0), ctypes.c_int(0)
    rc = lib.tg_bn_launch_geometry(n, c, hw, ctypes.byref(t), ctypes.byref(s))
    assert rc == 0, rc
    return t.value, s.value
