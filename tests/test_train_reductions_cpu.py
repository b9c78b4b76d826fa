"""No GPU: what tests/test_hip_train_reductions.py relies on.  The BatchNorm shape table selects the launch forms it
names (tg_bn_launch_geometry is a host function), the float64 references of tests/train_reductions_ref.py agree with
torch's own double-precision ops, and exact-sum inputs give one bit pattern under every fp32 summation order."""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import tecogan_pytorch_amd  # noqa: F401
from tecogan_pytorch_amd import _lib as L
from tests import train_reductions_ref as R


@pytest.mark.parametrize('shape,expect', R.BN_CASES, ids=['x'.join(map(str, s)) for s, _ in R.BN_CASES])
def test_bn_shape_table_selects_the_stated_launch_form(shape, expect):
    n, c, h, w = shape
    threads, slices, vec = expect
    assert R.bn_geometry(L.lib(), n, c, h * w) == (threads, slices), \
        f'{shape} no longer reaches the {threads}-thread / {slices}-slice path: choose another shape for that row'
    assert ((h * w) % 4 == 0) == vec
    assert n % slices == 0


def test_bn_shape_table_covers_every_form():
    lib = L.lib()
    forms = {(R.bn_geometry(lib, n, c, h * w), v) for (n, c, h, w), (_, _, v) in R.BN_CASES}
    assert {((256, 1), True), ((1024, 1), True), ((1024, 1), False)} <= forms
    assert {s for (_, s), _ in forms} >= {1, 2, 6, 8}
    assert any(s > 1 and not v for (_, s), v in forms)                     # sliced + scalar
    # four-image loop alone / tail alone / both, also at a non-zero slice base
    per_slice = [(n // s, v) for (n, _, _, _), (_, s, v) in R.BN_CASES if v]
    assert {m for m, _ in per_slice} >= {1, 3, 4, 5, 7}
    n, c, h, w = R.BN_CASES[-1][0]
    assert n * c * h * w // 4 > R.GRID_CAP_THREADS                         # 16-byte apply kernels take a second trip
    assert lib.tg_bn_launch_geometry(4, 4, 16, None, None) == -2
    t, s = ctypes.c_int(), ctypes.c_int()
    assert lib.tg_bn_launch_geometry(0, 4, 16, ctypes.byref(t), ctypes.byref(s)) != 0


@pytest.mark.parametrize('shape', [(3, 4, 5, 6), (2, 3, 7, 4)])
def test_references_match_torch_double(shape):
    g = torch.Generator().manual_seed(shape[0])
    n, c, h, w = shape
    x = torch.randn(shape, generator=g, dtype=torch.float64).requires_grad_(True)
    gamma = (torch.rand(c, generator=g, dtype=torch.float64) + 0.5).requires_grad_(True)
    beta = torch.randn(c, generator=g, dtype=torch.float64).requires_grad_(True)
    dy = torch.randn(shape, generator=g, dtype=torch.float64)
    rm0, rv0 = torch.randn(c, generator=g, dtype=torch.float64), torch.rand(c, generator=g, dtype=torch.float64) + 0.5
    rm, rv = rm0.clone(), rv0.clone()
    mom = float(np.float32(0.1))
    yt = F.leaky_relu(F.batch_norm(x, rm, rv, gamma, beta, training=True, momentum=mom, eps=1e-5), 0.2)
    yt.backward(dy)
    y, mean, var, invstd = R.bn_fwd_ref(x.detach(), gamma.detach(), beta.detach())
    assert (y - yt.detach()).abs().max() <= 1e-12
    rmr, rvr = R.bn_running_ref(rm0, rv0, mean, var, n * h * w, 0.1)
    assert (rmr - rm).abs().max() <= 1e-12 and (rvr - rv).abs().max() <= 1e-12
    dx, dgamma, dbeta, _, _ = R.bn_bwd_ref(x.detach(), y, dy, gamma.detach(), mean, invstd)
    assert (dx - x.grad).abs().max() <= 1e-12
    assert (dgamma - gamma.grad).abs().max() <= 1e-12 and (dbeta - beta.grad).abs().max() <= 1e-12

    # BCE with logits / LSGAN
    lg = (torch.randn(shape, generator=g, dtype=torch.float64) * 4).requires_grad_(True)
    for tgt in (0.0, 1.0):
        lg.grad = None
        F.binary_cross_entropy_with_logits(lg, torch.full_like(lg, tgt), reduction='sum').backward()
        t0, sx, _, gr = R.bce_ref(lg.detach(), tgt)
        ref = F.binary_cross_entropy_with_logits(lg.detach(), torch.full_like(lg, tgt), reduction='none')
        assert (t0 - ref).abs().max() <= 1e-12 and (gr - lg.grad).abs().max() <= 1e-12
        lg.grad = None
        ((lg - tgt) ** 2).sum().backward()
        t0, _, lsig, gr = R.bce_ref(lg.detach(), tgt, lsgan=True)
        assert (t0 - (lg.detach() - tgt) ** 2).abs().max() <= 1e-12 and (gr - lg.grad).abs().max() <= 1e-12
        assert (lsig - torch.log(torch.sigmoid(lg.detach()) + float(np.float32(1e-8)))).abs().max() <= 1e-12

    # a saturated logit: sigmoid(-90) + 1e-8 is 1e-8, its logarithm finite
    _, _, lsig, _ = R.bce_ref(torch.tensor([-90.0, 90.0]), 1.0)
    assert abs(lsig[0].item() - math.log(float(np.float32(1e-8)))) < 1e-12 and abs(lsig[1].item() - 1e-8) < 1e-9
    # cosine similarity over dim 1 (with a pixel below eps and an all-zero pixel)
    a = torch.randn(shape, generator=g, dtype=torch.float64)
    b = torch.randn(shape, generator=g, dtype=torch.float64)
    a[0, :, 0, 0] = 1e-10
    a[0, :, 0, 1] = 0.0
    a.requires_grad_(True)
    terms, da = R.cosine_ref(a.detach(), b)
    assert (terms - (1.0 - F.cosine_similarity(a.detach(), b, dim=1, eps=1e-8))).abs().max() <= 1e-12
    # gradient: F.cosine_similarity where no norm is clamped (its backward of a clamped norm depends on the torch
    # version: newer ones clamp under no_grad) ...
    (1.0 - F.cosine_similarity(a, b, dim=1, eps=1e-8)).sum().backward()
    free = (a.detach().norm(dim=1, keepdim=True) > 1e-8).expand_as(a)
    assert (da - a.grad)[free].abs().max() <= 1e-12
    # ... and everywhere the formula the loss is defined by, x / clamp_min(|x|, eps), through autograd: a clamped
    # norm passes no gradient, an all-zero pixel gets b / (eps |b|)
    a.grad = None
    an = a / a.norm(dim=1, keepdim=True).clamp_min(1e-8)
    bn = b / b.norm(dim=1, keepdim=True).clamp_min(1e-8)
    (1.0 - (an * bn).sum(1)).sum().backward()
    assert torch.isfinite(a.grad).all()
    assert ((da - a.grad).abs() <= 1e-12 * a.grad.abs().clamp_min(1.0)).all()

    # Charbonnier, L1, MSE and Adam against autograd / torch.optim
    xx = torch.randn(shape, generator=g, dtype=torch.float64).requires_grad_(True)
    yy = torch.randn(shape, generator=g, dtype=torch.float64)
    torch.sqrt((xx - yy) ** 2 + 1e-6).sum().backward()
    r, gr = R.charbonnier_ref(xx.detach(), yy)
    assert (gr - xx.grad).abs().max() <= 1e-12 and abs(r.sum() - torch.sqrt((xx.detach() - yy) ** 2 + 1e-6).sum()) <= 1e-10
    for mode, fn in ((1, F.l1_loss), (2, F.mse_loss)):
        xx.grad = None
        fn(xx, yy, reduction='sum').backward()
        t, gr = R.pixel_ref(xx.detach(), yy, mode)
        assert (gr - xx.grad).abs().max() <= 1e-12 and abs(t.sum() - fn(xx.detach(), yy, reduction='sum')) <= 1e-10
    p = torch.nn.Parameter(torch.randn(37, generator=g, dtype=torch.float64))
    p0 = p.detach().clone()
    hp = [float(np.float32(s)) for s in (1e-3, 0.9, 0.999, 1e-8, 0.01)]
    opt = torch.optim.Adam([p], lr=hp[0], betas=(hp[1], hp[2]), eps=hp[3], weight_decay=hp[4])
    m = torch.zeros(37, dtype=torch.float64); v = torch.zeros(37, dtype=torch.float64)
    pr = p0
    for step in (1, 2, 3):
        p.grad = torch.randn(37, generator=g, dtype=torch.float64)
        pr, m, v = R.adam_ref(pr, p.grad, m, v, 1e-3, 0.9, 0.999, 1e-8, 0.01, step)
        opt.step()
        assert (pr - p.detach()).abs().max() <= 1e-12


@pytest.mark.parametrize('denom,kmax', [(8, 8), (2, 4)])
def test_exact_sum_inputs_are_order_independent(denom, kmax):
    """262144 values j / denom: per-thread strides of 256 and 1024, 1 / 2 / 8 slices, a pairwise tree and the plain
    sequential order all give the fp32 image of the float64 sum, bit for bit; so do the sums of squares."""
    x = R.exact_values(5, (262144,), denom, kmax).numpy()
    assert len(x) * kmax * kmax <= 2 ** 24          # integers up to 2^24 (in units of 1 / denom^2) are fp32 numbers
    for v in (x, x * x):
        want = np.float32(v.astype(np.float64).sum())
        assert float(want) == v.astype(np.float64).sum()                 # the exact sum is an fp32 number
        got = [R.sum_f32_strided(v, t, ch) for t in (256, 1024) for ch in (1, 2, 8)]
        got += [R.sum_f32_pairwise(v), R.sum_f32_sequential(v)]
        assert {g.tobytes() for g in got} == {want.tobytes()}, (got, want)
    # generic data does depend on the order (the generator, not the summation code, is what makes the sums equal)
    r = np.random.RandomState(0).uniform(-1, 1, 262144).astype(np.float32)
    assert len({R.sum_f32_strided(r, 256).tobytes(), R.sum_f32_strided(r, 1024, 8).tobytes(),
                R.sum_f32_sequential(r).tobytes()}) > 1
