"""A torch statement of conv3x3(bilinear_x2(x)) with the channel mix at the LOW resolution (csrc/tg_upconv.hip):

    z[ky, kx, o][a, b]       = sum over c of W[o, c, ky, kx] * x[c, a, b]
    conv3x3(up2(x))[o, Y, X] = bias[o] + sum over (ky, kx) of inside(Y+ky-1, X+kx-1) * up2(z[ky, kx, o])[Y+ky-1, X+kx-1]

`inside` is the conv's zero padding on the up-sampled map; up2 is F.interpolate(scale_factor=2, mode='bilinear',
align_corners=False) written out: up[2a] = 1/4 v[a-1] + 3/4 v[a], up[2a+1] = 3/4 v[a] + 1/4 v[a+1], indices clamped.
Any dtype, CPU or GPU.  tests/test_upconv_cpu.py holds it against F.interpolate + F.conv2d in fp64 and shows that the
two ways to get it wrong (a tap shifted the other way, a border that is not clamped) do not pass; the GPU tests use it
as the reference of the kernels' intermediate z and of the whole.
"""
import torch
import torch.nn.functional as F


def up2_axis(v, dim, clamp=True):
    """Bilinear x2 along `dim` (a non-negative index)."""
    n = v.shape[dim]
    idx = torch.arange(n, device=v.device)
    lo = v.index_select(dim, (idx - 1).clamp(min=0))
    hi = v.index_select(dim, (idx + 1).clamp(max=n - 1))
    if not clamp:        # the wrong border: zeros outside the map instead of the edge value
        keep = torch.ones(n, dtype=v.dtype, device=v.device)
        shape = [1] * v.dim()
        shape[dim] = n
        first, last = keep.clone(), keep.clone()
        first[0], last[n - 1] = 0, 0
        lo, hi = lo * first.view(shape), hi * last.view(shape)
    even = 0.25 * lo + 0.75 * v
    odd = 0.75 * v + 0.25 * hi
    return torch.stack((even, odd), dim=dim + 1).flatten(dim, dim + 1)


def up2(v, clamp=True):
    """(..., h, w) -> (..., 2h, 2w): along x, then along y, as the combine kernel blends."""
    return up2_axis(up2_axis(v, v.dim() - 1, clamp), v.dim() - 2, clamp)


def tap_planes(x, w):
    """z (n, 9 * cout, h, w), plane (ky * 3 + kx) * cout + o: what tg_upconv_tap_gemm writes."""
    n, _, h, wd = x.shape
    cout = w.shape[0]
    return torch.einsum('ocyx,ncab->nyxoab', w, x).reshape(n, 9 * cout, h, wd)


def combine(z, bias, cout, slope=None, clamp=True, shift=1):
    """What tg_upconv_combine computes from z.  shift = -1: every tap moved the wrong way (a bug the tests must catch)."""
    n, _, h, wd = z.shape
    zu = F.pad(up2(z.reshape(n, 3, 3, cout, h, wd), clamp), (1, 1, 1, 1))
    y = torch.zeros(n, cout, 2 * h, 2 * wd, dtype=z.dtype, device=z.device)
    if bias is not None:
        y = y + bias.view(1, cout, 1, 1)
    for ky in range(3):
        for kx in range(3):
            oy, ox = 1 + shift * (ky - 1), 1 + shift * (kx - 1)
            y = y + zu[:, ky, kx, :, oy:oy + 2 * h, ox:ox + 2 * wd]
    return y if slope is None else torch.where(y >= 0, y, y * slope)


def factored(x, w, bias, slope=None, clamp=True, shift=1):
    return combine(tap_planes(x, w), bias, w.shape[0], slope, clamp, shift)


def composed(x, w, bias, slope=None):
    """The reference: the up-sampled tensor, then the conv."""
    y = F.conv2d(F.interpolate(x, scale_factor=2, mode='bilinear', align_corners=False), w, bias, padding=1)
    return y if slope is None else torch.where(y >= 0, y, y * slope)
