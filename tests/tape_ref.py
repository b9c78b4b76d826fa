"""Helpers shared by tests/test_tape_ref_cpu.py (which checks them on the CPU), tests/test_hip_warp_bwd.py and
tests/test_hip_tape.py: inputs that keep every kinked op (bilinear sampling, max-pool, ReLU / LeakyReLU) away from
its kinks, and float64 references with the quantities the rounding bounds of the warp gradient are made of.
Everything here runs on the CPU."""
import types

import numpy as np
import torch

from oracle import tecogan_oracle as O
from tests.train_reductions_ref import U, gamma_k

# Rounded fp32 operations between `flow` and the sampling position `sx` in backward_warp_bwd_kernel
# (csrc/tg_train.hip; the same expression is tg_common.h: warp_coord):
#     gx = linspace_m1p1(px) + fx / halfx          fx / halfx (1), the addition (2)
#     ux = (gx + 1.0f) * halfx                     gx + 1 (3), the product (4)
# half = (size - 1) / 2 is exact, linspace_m1p1 reproduces the oracle's fp32 linspace bit for bit (the float64
# reference starts from the same fp32 values), the clip and floorf are exact and sx - floorf(sx) is exact (Sterbenz).
# Each of the four moves the position by at most u * (size - 1):  u |f / half| half = u |f|,  u |g| half,
# u |g + 1| half  and  u |ux|,  with |f|, |ux| <= size - 1 and |g|, |g + 1| <= 2 for an in-range target.
POS_OPS = 4


def pos_delta(size):
    """Largest distance between the kernel's fp32 sampling position and the float64 one along an axis of `size`."""
    return POS_OPS * U * (size - 1)


def kinkfree_flow(seed, n, h, w, out_frac):
    """Flow (n, 2, h, w) built from target sampling positions.  In-range targets are cell + k / 16, cell in
    [0, size - 2], k in [2, 14]: at least 1/8 pixel from every integer and from both clip limits.  Per axis,
    independently, round(out_frac * n h w) pixels (two at least when out_frac > 0) get a target outside the image,
    alternately at -0.5 - j / 4 and size - 1 + 0.5 + j / 4 (j in [0, 3]): clipped on each side.  flow = target -
    pixel coordinate: multiples of 1/16 below 2^12, exact in fp32.
    Returns (flow, clip_x, clip_y); the masks are boolean (n, h, w)."""
    r = np.random.RandomState(seed)
    npix = n * h * w
    out = []
    for size in (w, h):
        t = r.randint(0, size - 1, npix) + r.randint(2, 15, npix) / 16.0
        k = 0 if out_frac <= 0 else min(npix, max(2, int(round(out_frac * npix))))
        idx = r.permutation(npix)[:k]
        j = r.randint(0, 4, k) / 4.0
        t[idx] = np.where(np.arange(k) % 2 == 0, -0.5 - j, size - 1 + 0.5 + j)
        clip = np.zeros(npix, bool)
        clip[idx] = True
        out.append((t.reshape(n, h, w), clip.reshape(n, h, w)))
    (tx, cx), (ty, cy) = out
    fx = tx - np.arange(w).reshape(1, 1, w)
    fy = ty - np.arange(h).reshape(1, h, 1)
    flow = np.stack([fx, fy], 1)
    f32 = flow.astype(np.float32)
    assert (f32.astype(np.float64) == flow).all()
    return torch.from_numpy(f32), torch.from_numpy(cx), torch.from_numpy(cy)


def flow_targets(flow):
    """The target positions (x, y) a flow asks for, float64 (n, h, w) each."""
    n, _, h, w = flow.shape
    f = flow.double()
    return (f[:, 0] + torch.arange(w, dtype=torch.float64).view(1, 1, w),
            f[:, 1] + torch.arange(h, dtype=torch.float64).view(1, h, 1))


def act_ref(z64, y_dev, act):
    """float64 activation of the pre-activation z64 with the decision taken from the device's forward output y_dev:
    ReLU (1) z * (y_dev > 0), LeakyReLU (2) z * where(y_dev > 0, 1, 0.2), tanh * 24 (3) the smooth formula, 0 identity.
    Returns (y64, slack): slack is the largest |z64| among elements whose sign disagrees with the device's decision
    -- every caller asserts it is within the forward tolerance, so pinning cannot hide a wrong forward pass."""
    if act == 0:
        return z64, 0.0
    if act == 3:
        return torch.tanh(z64) * 24.0, 0.0
    pos = (y_dev.detach().cpu() > 0)
    slope = 0.0 if act == 1 else 0.2
    y = z64 * torch.where(pos, torch.ones((), dtype=z64.dtype), torch.full((), slope, dtype=z64.dtype))
    wrong = pos != (z64.detach() > 0)
    slack = z64.detach().abs()[wrong].max().item() if wrong.any() else 0.0
    return y, slack


def distinct_windows(seed, shape):
    """(n, c, h, w) max-pool input: every plane is a permutation of 0 .. h w - 1 scaled by 1 / 64 and centred, so
    any two values of a plane -- of a 2x2 window in particular -- are at least 1/64 apart: no tie, no near-tie."""
    n, c, h, w = shape
    r = np.random.RandomState(seed)
    p = np.stack([r.permutation(h * w) for _ in range(n * c)]).reshape(n, c, h, w)
    return torch.from_numpy(((p - (h * w) // 2) / 64.0).astype(np.float32))


def depth_to_space(y, s):
    """Inverse of the oracle's space_to_depth (plane (sy s + sx) c + ch)."""
    n, k, h, w = y.shape
    c = k // (s * s)
    return y.reshape(n, s, s, c, h, w).permute(0, 3, 4, 1, 5, 2).reshape(n, c, h * s, w * s)


def warp_bwd_ref(x, flow, dy, s2d=1):
    """float64 gradients of space_to_depth(backward_warp(x, flow), s2d) (s2d = 1: of backward_warp) by autograd on
    the oracle, and the per-element quantities the bounds of tests/test_hip_warp_bwd.py need, from the closed form
    of the same gradient (float64; tests/test_tape_ref_cpu.py holds the closed form to autograd):
      dimg, dflow          autograd
      clip_x, clip_y       (n, h, w) the position is clipped (no flow gradient)
      abs_img              scatter of |contribution| per image element
      count                contributions per image element (taps with a non-zero weight inside the image)
      sens_img             scatter of |g| (wy delta_x + wx delta_y): what a position error of pos_delta moves
      abs_fx, abs_fy       per pixel, the sum of absolute terms of the flow gradient's formula
      cross_fx, cross_fy   per pixel sum_ch |g| (|v01 - v00| + |v11 - v10|) and (|v10 - v00| + |v11 - v01|): the
                           sensitivity of d/dfx to the position along y, of d/dfy to the position along x."""
    n, c, h, w = x.shape
    xr = x.double().requires_grad_(True)
    fr = flow.double().requires_grad_(True)
    out = O.backward_warp(xr, fr)
    if s2d > 1:
        out = O.space_to_depth(out, s2d)
    out.backward(dy.double())
    g = (depth_to_space(dy, s2d) if s2d > 1 else dy).double()

    f = flow.double()
    lx = torch.from_numpy(O.linspace_m1_p1(w)).double().view(1, 1, w)
    ly = torch.from_numpy(O.linspace_m1_p1(h)).double().view(1, h, 1)
    hx, hy = (w - 1) / 2.0, (h - 1) / 2.0
    ux = (lx + f[:, 0] / hx + 1.0) * hx
    uy = (ly + f[:, 1] / hy + 1.0) * hy
    clip_x = (ux <= 0) | (ux >= w - 1)
    clip_y = (uy <= 0) | (uy >= h - 1)
    px, py = ux.clamp(0, w - 1), uy.clamp(0, h - 1)
    x0, y0 = px.floor(), py.floor()
    wx1, wy1 = px - x0, py - y0
    wx0, wy0 = 1.0 - wx1, 1.0 - wy1
    x0, y0 = x0.long(), y0.long()
    x1, y1 = x0 + 1, y0 + 1
    xd = x.double().reshape(n, c, h * w)

    def tap(yy, xx):
        ok = (xx <= w - 1) & (yy <= h - 1)
        idx = yy.clamp(max=h - 1) * w + xx.clamp(max=w - 1)
        v = torch.gather(xd, 2, idx.view(n, 1, h * w).expand(n, c, h * w)).view(n, c, h, w)
        return v * ok.unsqueeze(1), ok, idx
    v00, ok00, i00 = tap(y0, x0)
    v01, ok01, i01 = tap(y0, x1)
    v10, ok10, i10 = tap(y1, x0)
    v11, ok11, i11 = tap(y1, x1)
    ga = g.abs()
    WX0, WX1, WY0, WY1 = (t.unsqueeze(1) for t in (wx0, wx1, wy0, wy1))
    r = types.SimpleNamespace(dimg=xr.grad, dflow=fr.grad, clip_x=clip_x, clip_y=clip_y)
    r.formula_fx = (g * ((v01 - v00) * WY0 + (v11 - v10) * WY1)).sum(1) * (~clip_x)
    r.formula_fy = (g * ((v10 - v00) * WX0 + (v11 - v01) * WX1)).sum(1) * (~clip_y)
    r.abs_fx = (ga * ((v01.abs() + v00.abs()) * WY0 + (v11.abs() + v10.abs()) * WY1)).sum(1)
    r.abs_fy = (ga * ((v10.abs() + v00.abs()) * WX0 + (v11.abs() + v01.abs()) * WX1)).sum(1)
    r.cross_fx = (ga * ((v01 - v00).abs() + (v11 - v10).abs())).sum(1)
    r.cross_fy = (ga * ((v10 - v00).abs() + (v11 - v01).abs())).sum(1)

    dx_, dy_ = pos_delta(w), pos_delta(h)
    formula = torch.zeros(n, c, h * w, dtype=torch.float64)
    abs_img, sens, count = torch.zeros_like(formula), torch.zeros_like(formula), torch.zeros_like(formula)
    for (wy, wx, ok, idx) in ((WY0, WX0, ok00, i00), (WY0, WX1, ok01, i01), (WY1, WX0, ok10, i10), (WY1, WX1, ok11, i11)):
        okc = ok.unsqueeze(1).double()
        ix = idx.view(n, 1, h * w).expand(n, c, h * w)
        wgt = (wy * wx * okc).expand(n, c, h, w)
        formula.scatter_add_(2, ix, (g * wgt).reshape(n, c, -1))
        abs_img.scatter_add_(2, ix, (ga * wgt).reshape(n, c, -1))
        sens.scatter_add_(2, ix, (ga * (wy * dx_ + wx * dy_) * okc).reshape(n, c, -1))
        count.scatter_add_(2, ix, (wgt != 0).double().reshape(n, c, -1))
    r.formula_img = formula.view(n, c, h, w)
    r.abs_img, r.sens_img, r.count = abs_img.view(n, c, h, w), sens.view(n, c, h, w), count.view(n, c, h, w)
    return r


def flow_chain(c):
    """Rounded fp32 operations behind one component of the flow gradient in backward_warp_bwd_kernel, per pixel:
        wy0 = 1.f - wy1                                              1     (wy1 = sy - floorf(sy) is exact)
        per channel  gsx += g * ((v01 - v00) * wy0 + (v11 - v10) * wy1)
                     two differences, two products, their sum, the product with g, the accumulation: 7 c
        dflow = gsx * mx                                             exact (mx is 0 or 1)
    A fused multiply-add only removes roundings.  Every term of the sum therefore carries at most 7 c + 1 factors
    (1 + d), |d| <= u: the result is within gamma_(7 c + 1) * (sum of absolute terms) of the float64 value at the
    same position."""
    return 7 * c + 1


def flow_bound(ref, c, h, w):
    """Per-pixel bounds (x, y) of the flow gradient: gamma_k * S + delta * S2 (module docstring of
    tests/test_hip_warp_bwd.py).  d/dfx depends on the position only through wy, d/dfy only through wx."""
    k = gamma_k(flow_chain(c))
    return k * ref.abs_fx + pos_delta(h) * ref.cross_fx, k * ref.abs_fy + pos_delta(w) * ref.cross_fy


def img_bound(ref, prefill=None):
    """Per-element bound of the image gradient.  One contribution is g * wy * wx: two products, and each weight of
    the form 1.f - w1 is one more rounding (4 at most); the m contributions of an element then meet in m - 1 atomic
    additions in any order (the first lands on an exact zero): gamma_(m + 3) * A.  Accumulating onto a non-zero
    pre-fill p is one more addition and p is one more term: gamma_(m + 4) * (A + |p|)."""
    m = ref.count
    if prefill is None:
        return gamma_k(m + 3) * ref.abs_img + ref.sens_img
    return gamma_k(m + 4) * (ref.abs_img + prefill.double().abs()) + ref.sens_img


# (n, c, h, w) of the warp-gradient tests: the smallest shapes that reach each geometry of the launch (64 columns x
# 4 rows per block, blockIdx.z = n)
WARP_SHAPES = [
    (1, 1, 2, 2),        # the smallest legal image
    (2, 3, 17, 23),      # one column block, the last row group partial
    (2, 3, 18, 70),      # two column blocks, the second partial; h, w even: space_to_depth 2
    (1, 3, 8, 132),      # three column blocks; space_to_depth 4
    (3, 2, 5, 64),       # exactly one full column block, h not a multiple of 4
]
OUT_FRAC = 0.15


def warp_inputs(seed, shape, out_frac=OUT_FRAC, s2d=1):
    """(x, flow, dy, clip_x, clip_y) of one warp-gradient case; dy in the space_to_depth layout when s2d > 1."""
    n, c, h, w = shape
    r = np.random.RandomState(seed)
    x = torch.from_numpy(r.uniform(0, 1, shape).astype(np.float32))
    dy = torch.from_numpy(r.uniform(-1, 1, (n, c * s2d * s2d, h // s2d, w // s2d)).astype(np.float32))
    flow, cx, cy = kinkfree_flow(seed + 1, n, h, w, out_frac)
    return x, flow, dy, cx, cy
