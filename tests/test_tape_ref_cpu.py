"""tests/tape_ref.py on the CPU: the inputs have the margins they promise, the closed form behind the warp
gradient's bounds is the oracle's autograd, and the reference alone (the oracle in fp32 against itself in float64)
stays inside the bounds the kernels are held to in tests/test_hip_warp_bwd.py -- at every pixel, none left out."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import tecogan_oracle as O
from tests import tape_ref as TR

CASES = [(shape, TR.OUT_FRAC, 1) for shape in TR.WARP_SHAPES] + \
        [((2, 3, 17, 23), 1.0, 1), ((2, 3, 17, 23), 0.0, 1), ((2, 3, 18, 70), TR.OUT_FRAC, 2),
         ((1, 3, 8, 132), TR.OUT_FRAC, 4), ((1, 3, 8, 132), TR.OUT_FRAC, 2), ((1, 1, 2, 2), TR.OUT_FRAC, 2)]


@pytest.mark.parametrize('shape,out_frac,s2d', CASES)
def test_kinkfree_flow_margins(shape, out_frac, s2d):
    n, c, h, w = shape
    flow, cx, cy = TR.kinkfree_flow(7, n, h, w, out_frac)
    assert flow.dtype == torch.float32 and flow.shape == (n, 2, h, w)
    tx, ty = TR.flow_targets(flow)
    for t, clip, size in ((tx, cx, w), (ty, cy, h)):
        inside = t[~clip]
        if inside.numel():
            assert (inside - inside.round()).abs().min() >= 0.125
            assert inside.min() >= 0.125 and inside.max() <= size - 1 - 0.125
        out = t[clip]
        lo, hi = out[out < 0], out[out > 0]
        assert lo.numel() + hi.numel() == out.numel()
        if out_frac > 0:
            assert lo.numel() > 0 and hi.numel() > 0                  # both clip sides, on this axis
            assert lo.max() <= -0.5 and hi.min() >= size - 1 + 0.5
        else:
            assert out.numel() == 0
        if out_frac >= 1.0:
            assert clip.all()


@pytest.mark.parametrize('shape,out_frac,s2d', CASES)
def test_reference_alone_stays_inside_the_bounds(shape, out_frac, s2d):
    n, c, h, w = shape
    x, flow, dy, cx, cy = TR.warp_inputs(11, shape, out_frac, s2d)
    ref = TR.warp_bwd_ref(x, flow, dy, s2d)
    assert torch.equal(ref.clip_x, cx) and torch.equal(ref.clip_y, cy)
    # the closed form the bounds are computed from IS the oracle's gradient
    assert (ref.formula_fx - ref.dflow[:, 0]).abs().max() <= 1e-13 * max(1.0, ref.dflow.abs().max().item())
    assert (ref.formula_fy - ref.dflow[:, 1]).abs().max() <= 1e-13 * max(1.0, ref.dflow.abs().max().item())
    assert (ref.formula_img - ref.dimg).abs().max() <= 1e-13 * max(1.0, ref.dimg.abs().max().item())
    assert (ref.dflow[:, 0][cx] == 0).all() and (ref.dflow[:, 1][cy] == 0).all()
    assert (ref.dimg[ref.count == 0] == 0).all()
    # fp32 autograd of the oracle, every pixel
    xr, fr = x.clone().requires_grad_(True), flow.clone().requires_grad_(True)
    out = O.backward_warp(xr, fr)
    if s2d > 1:
        out = O.space_to_depth(out, s2d)
    out.backward(dy)
    bx, by = TR.flow_bound(ref, c, h, w)
    ex = (fr.grad[:, 0].double() - ref.dflow[:, 0]).abs()
    ey = (fr.grad[:, 1].double() - ref.dflow[:, 1]).abs()
    assert (ex <= bx).all() and (ey <= by).all(), ((ex / bx.clamp_min(1e-300)).max(), (ey / by.clamp_min(1e-300)).max())
    assert (fr.grad[:, 0][cx] == 0).all() and (fr.grad[:, 1][cy] == 0).all()
    ei = (xr.grad.double() - ref.dimg).abs()
    bi = TR.img_bound(ref)
    assert (ei <= bi).all(), (ei / bi.clamp_min(1e-300)).max()
    assert (xr.grad[ref.count == 0] == 0).all()
    if out_frac >= 1.0:
        assert not fr.grad.any() and not ref.dflow.any()


def test_distinct_windows_gap():
    for shape in [(2, 5, 9, 13), (1, 3, 2, 2), (2, 4, 7, 24)]:
        x = TR.distinct_windows(3, shape)
        n, c, h, w = shape
        win = x[:, :, :h // 2 * 2, :w // 2 * 2].reshape(n, c, h // 2, 2, w // 2, 2).permute(0, 1, 2, 4, 3, 5)
        win = win.reshape(n, c, h // 2, w // 2, 4).double()
        s, _ = win.sort(-1)
        assert (s[..., 1:] - s[..., :-1]).min() >= 1.0 / 64


def test_act_ref_reproduces_torch():
    z = torch.from_numpy(np.random.RandomState(5).uniform(-2, 2, (3, 5, 7, 9)))
    for act, fn in ((0, lambda t: t), (1, torch.relu), (2, lambda t: F.leaky_relu(t, 0.2)),
                    (3, lambda t: torch.tanh(t) * 24)):
        zr = z.clone().requires_grad_(True)
        want = fn(zr)
        got, slack = TR.act_ref(zr, want.detach(), act)
        assert torch.equal(got, want) and slack == 0.0
        g1, = torch.autograd.grad(got.sum(), zr, retain_graph=True)
        g2, = torch.autograd.grad(want.sum(), zr)
        assert torch.equal(g1, g2)
    # a decision that disagrees with the sign is reported with the size of the value it was taken on
    y = torch.relu(z)
    y[0, 0, 0, 0] = 1.0 if z[0, 0, 0, 0] <= 0 else 0.0
    _, slack = TR.act_ref(z, y, 1)
    assert slack == z[0, 0, 0, 0].abs().item()
