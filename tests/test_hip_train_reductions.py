"""The kernels of csrc/tg_train.hip against closed-form float64 references on every launch path: the three forms of
bn_sweep, 256- and 1024-thread blocks, sliced launches and their merges, the 16-byte and scalar apply kernels, the
mid-plane slices of bias_grad and the second trip of every grid-stride loop.

Two kinds of input.  EXACT-SUM inputs (values j / 8, sized so that every partial sum fits 24 bits): any summation
order gives the exact result, so sums must equal fp32(float64 reference) bit for bit.  GENERIC inputs: compared with
float64 under a bound derived in each test's docstring from u = 2^-24 and gamma_k = k u / (1 - k u), k = the longest
chain of additions of that launch (elements per thread + 6 wave shuffles + waves per block + slices / atomic adds),
computed from the launch geometry.  No bound comes from what a kernel happened to produce; each test prints
`[measured]` lines (worst error, its bound) -- run with -s to see them.

Library functions (u = 2^-24).  No accuracy table ships with the toolchain, so each was measured alone against
double on an MI355X over the range used here (4M points each, worst relative error): expf 1.38 u on [-87, 88],
logf 2.70 u on [1e-8, 1.001], log1pf 1.04 u on [1e-38, 1]; TWICE that is allowed (E_EXP, E_LOG, E_LOG1P).  sqrtf and
1.0f / x measured 0.500 ulp, i.e. correctly rounded: the format's own bound, 1 u, is used for them."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import tecogan_oracle as O
from tests import train_reductions_ref as R

U = R.U
gk = R.gamma_k
# allowed relative error of the library functions, in units of u (see the module docstring)
E_SQRT, E_DIV, E_EXP, E_LOG, E_LOG1P = 1.0, 1.0, 2.8, 5.4, 2.1
FLT_MIN = 2.0 ** -126               # results below the normal range may be flushed to zero
N_BIG = 4096 * 256 + 777            # past grid_for()'s cap: the stride loop takes a second trip, ragged end
N_SMALL = 257


@pytest.fixture(scope='module')
def ops():
    import tecogan_pytorch_amd.ops as ops_
    return ops_


@pytest.fixture(scope='module')
def lib():
    from tecogan_pytorch_amd import _lib
    return _lib.lib()


def rs(seed):
    return np.random.RandomState(seed)


def f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def place(t, offset=False, fill=None):
    """t on the GPU; offset: a contiguous view one float into a larger buffer (4-byte aligned, not 16)."""
    if not offset:
        d = t.cuda().contiguous()
        assert d.data_ptr() % 16 == 0
    else:
        buf = torch.empty(t.numel() + 8, dtype=torch.float32, device='cuda')
        d = buf[1:1 + t.numel()].view(t.shape)
        d.copy_(t)
        assert d.is_contiguous() and d.data_ptr() % 16 == 4
    if fill is not None:
        d.fill_(fill)
    return d


def check(name, got, ref, bound):
    """|got - ref| <= bound element-wise (float64); prints the worst error next to its bound."""
    got = got.detach().cpu().double()
    ref = torch.as_tensor(ref).detach().cpu().double().reshape(got.shape)
    bound = torch.broadcast_to(torch.as_tensor(bound, dtype=torch.float64), got.shape).reshape(-1)
    got, ref = got.reshape(-1), ref.reshape(-1)
    assert torch.isfinite(got).all(), f'{name}: non-finite output'
    err = (got - ref).abs()
    ratio = err / bound.clamp_min(1e-300)
    i = int(ratio.argmax())
    print(f'[measured] {name}: err {err[i].item():.3e} bound {bound[i].item():.3e} ({ratio[i].item():.3f} of it); '
          f'max err {err.max().item():.3e}')
    assert (err <= bound).all(), f'{name}: err {err[i].item():.3e} > bound {bound[i].item():.3e} at {i}'


def bits_equal(name, got, ref64):
    """got == fp32(ref64) bit for bit."""
    want = ref64.detach().cpu().double().float()
    got = got.detach().cpu()
    same = got.view(torch.int32) == want.view(torch.int32)
    both_zero = (got == 0) & (want == 0)
    bad = ~(same | both_zero)
    print(f'[measured] {name}: {int(bad.sum())} of {got.numel()} elements differ from fp32(fp64)')
    assert not bad.any(), f'{name}: {int(bad.sum())} elements differ, first at {int(bad.reshape(-1).nonzero()[0])}: ' \
                          f'{got.reshape(-1)[bad.reshape(-1)][0].item()!r} vs {want.reshape(-1)[bad.reshape(-1)][0].item()!r}'


# =================================================================================================
# BatchNorm + LeakyReLU, fused entry points
# =================================================================================================
def bn_inputs(shape, variant, seed):
    n, c, h, w = shape
    r = rs(seed)
    gamma = f32(r.uniform(0.5, 1.5, c) * np.where(np.arange(c) % 3 == 2, -1.0, 1.0))
    if variant == 'generic':
        x = f32(r.normal(0, 1.5, shape) + r.uniform(-1, 1, (1, c, 1, 1)))
        beta = f32(r.normal(0, 0.5, c))
        dy = f32(r.normal(0, 1, shape))
    elif variant == 'exact':
        assert n * h * w * 8 <= 2 ** 24                       # sums of j / 8, |j| <= 8, in units of 1 / 8
        x = R.exact_values(seed, shape)
        beta = torch.full((c,), 100.0)
        dy = R.exact_values(seed + 1, shape)
    else:                                                     # 'offset': mean 50, std 0.05
        sign = np.where(np.arange(c) % 2 == 1, -1.0, 1.0).reshape(1, c, 1, 1)
        x = f32(50.0 * sign + r.normal(0, 0.05, shape))
        beta = f32(r.normal(0, 0.5, c))
        dy = f32(r.normal(0, 1, shape))
    return x, gamma, beta, dy


BN_RUNS = [(s, e, False) for s, e in R.BN_CASES] + \
          [(s, (e[0], e[1], False), True) for s, e in R.BN_CASES if s in ((7, 3, 48, 40), (2, 3, 128, 256))]


@pytest.mark.parametrize('variant', ['generic', 'exact', 'offset'])
@pytest.mark.parametrize('shape,expect,unaligned', BN_RUNS,
                         ids=['x'.join(map(str, s)) + ('-unaligned' if o else '') for s, _, o in BN_RUNS])
def test_bn_lrelu_train_fwd_bwd(ops, lib, shape, expect, unaligned, variant):
    """ops.bn_lrelu_train_fwd / _bwd on every launch form (the row's form is asked of tg_bn_launch_geometry first).

    k = elements per thread of bn_sweep + 6 + threads / 64 + slices (if sliced).  A = mean |x| of the channel.
      mean:    tot = fl(sum x) within gamma_k cnt A; / cnt (and / slices) one rounding each: gamma_{k+2} A.
      invstd:  the second pass sums (x - m)^2 around the COMPUTED mean m: sum (x-m)^2 = cnt var + cnt (m-mu)^2, so the
               mean's error enters squared, delta^2 / var with delta = gamma_k max|x|; the sum itself gamma_k; halved by
               the square root; + 2 u for sqrtf and the division: 1/2 (delta^2 / var + gamma_k) + 2 u, for every row.
      var:     (the running variance) the same without the root, with delta = gamma_{k+2} max|x| and the roundings of
               x - m, the square (3 u) and / cnt counted: delta^2 / var + gamma_k + (r - 1) u, r = 5 (the sliced merge
               adds d, d^2, cnt_r *, + : r = 9).
      running: T1 = (1 - mom) run0 (1 - mom rounded, product, final add: 3 u), T2 = mom * stat (stat's bound, product(s),
               final add): mean: mom B_mean + 2 u |T2|; var: (rel var bound + 4 u) |T2| (var * cnt / (cnt - 1): 2 more).
      y:       v = (x - m) is ga + be, z = v - be: |ga IS| B_mean + |z| (B_is + 3 u) + u |v|; slope: + u |y|.
    Backward, as a function of ITS inputs (the y, mean, invstd the forward produced), dz = dy or fl(0.2 dy):
      dbeta  = sum dz: gamma_{k+1} sum |dz|;   dgamma = sum dz xhat: gamma_{k+4} sum |dz xhat| (x - mu, * is, dz, product);
               both + u |result| for the wrapper's accumulation onto the non-zero start value.
      dx = gs (dz - s0 ic - xhat s1 ic): |gs| (B_s0 + |xhat| B_s1) / cnt + u |gs| (5 |dz| + 6 |s0| / cnt + 8 |xhat s1| / cnt)
               (roundings met by each term: gs, slope, ic = 1 / cnt, products, two subtractions, final product).
    'exact': beta = 100 makes every y positive, so dz = dy and sum x, sum dz are exact: dbeta bit-equal, mean within
    1 ulp (slices + 2 when sliced: one division per slice mean, the sum, the division by slices).
    'offset' (mean 50, std 0.05) fails any E[x^2] - mean^2 formulation (cancellation 50^2 / 0.0025 = 1e6 u) and a
    Chan merge with a wrong count or cross term."""
    n, c, h, w = shape
    hw, cnt = h * w, n * h * w
    threads, slices, vec = expect
    assert R.bn_geometry(lib, n, c, hw) == (threads, slices), f'{shape} no longer reaches this launch form'
    vec = vec and not unaligned
    x, gamma, beta, dy = bn_inputs(shape, variant, 11 + n + c)
    eps, mom, slope = 1e-5, 0.1, 0.2
    rm0, rv0 = f32(rs(3).normal(0, 1, c)), f32(rs(4).uniform(0.5, 2, c))
    xd, dyd = place(x, unaligned), place(dy, unaligned)
    yd = place(torch.empty(shape), unaligned, fill=float('nan'))
    dxd = place(torch.empty(shape), unaligned, fill=float('nan'))
    rm, rv = rm0.cuda(), rv0.cuda()
    gd, bd = gamma.cuda(), beta.cuda()
    y, mean, invstd = ops.bn_lrelu_train_fwd(xd, gd, bd, rm, rv, momentum=mom, eps=eps, slope=slope, out=yd)
    assert y.data_ptr() == yd.data_ptr()

    yr, mr, vr, isr = R.bn_fwd_ref(x, gamma, beta, eps, slope)
    k = R.block_chain(R.bn_sweep_chain(n // slices, hw, threads, vec), threads) + (slices if slices > 1 else 0)
    xa = x.double().abs()
    A, xmax = xa.mean((0, 2, 3)), xa.amax((0, 2, 3))
    b_mean = gk(k + 2) * A
    delta = gk(k + 2) * xmax
    r_ = 9 if slices > 1 else 5
    rel_var = delta ** 2 / vr + gk(k) + (r_ - 1) * U
    delta_i = gk(k) * xmax
    b_is_rel = 0.5 * (delta_i ** 2 / vr + gk(k)) + 2 * U
    tag = f'bn {shape} {variant}{" unaligned" if unaligned else ""} k={k}'
    check(f'{tag} mean', mean, mr, b_mean)
    check(f'{tag} invstd', invstd, isr, b_is_rel * isr)
    rmr, rvr = R.bn_running_ref(rm0, rv0, mr, vr, cnt, mom)
    m32 = float(np.float32(mom))
    check(f'{tag} running_mean', rm, rmr, 3 * U * ((1 - m32) * rm0.double()).abs() + m32 * b_mean + 2 * U * (m32 * mr).abs())
    t2 = m32 * vr * cnt / (cnt - 1.0)
    check(f'{tag} running_var', rv, rvr, 3 * U * ((1 - m32) * rv0.double()).abs() + (rel_var + 4 * U) * t2)
    V = lambda t: t.double().view(1, c, 1, 1)
    z = (x.double() - V(mr)) * V(isr) * V(gamma)
    v = z + V(beta)
    err_v = (V(gamma) * V(isr)).abs() * V(b_mean) + z.abs() * (V(b_is_rel) + 3 * U) + U * v.abs()
    check(f'{tag} y', y, yr, torch.where(v < -err_v, slope * err_v, err_v) + U * yr.abs())

    # backward from the forward's own outputs
    dg0, db0 = R.exact_values(7, (c,)) * 4, R.exact_values(8, (c,)) * 4
    dgamma, dbeta = dg0.cuda(), db0.cuda()
    dx = ops.bn_lrelu_train_bwd(xd, y, dyd, gd, mean, invstd, dgamma=dgamma, dbeta=dbeta, need_dx=True, slope=slope, dx_out=dxd)
    assert dx.data_ptr() == dxd.data_ptr()
    dxr, dgr, dbr, dz, xhat = R.bn_bwd_ref(x, y.cpu(), dy, gamma, mean.cpu(), invstd.cpu(), slope)
    b_s0 = gk(k + 1) * dz.abs().sum((0, 2, 3))
    b_s1 = gk(k + 4) * (dz * xhat).abs().sum((0, 2, 3))
    check(f'{tag} dbeta', dbeta, db0.double() + dbr, b_s0 + U * (db0.double() + dbr).abs())
    check(f'{tag} dgamma', dgamma, dg0.double() + dgr, b_s1 + U * (dg0.double() + dgr).abs())
    gs = (V(gamma) * V(invstd.cpu())).abs()
    b_dx = gs * (V(b_s0) + xhat.abs() * V(b_s1)) / cnt + \
        U * gs * (5 * dz.abs() + 6 * V(dbr).abs() / cnt + 8 * (xhat * V(dgr)).abs() / cnt)
    check(f'{tag} dx', dx, dxr, b_dx)

    if variant == 'exact':
        assert (y > 0).all()
        bits_equal(f'{tag} dbeta (exact)', dbeta, db0.double() + dy.double().sum((0, 2, 3)))
        ulps = R.ulp_distance(mean.cpu().numpy(), mr.float().numpy()).max()
        print(f'[measured] {tag} mean (exact): {ulps:.2f} ulp')
        assert ulps <= (slices + 2 if slices > 1 else 1)


# =================================================================================================
# SyncBN halves without a process group
# =================================================================================================
@pytest.mark.parametrize('world', [2, 3, 8])
@pytest.mark.parametrize('part', [(2, 4, 64, 128), (5, 3, 9, 7)], ids=['2x4x64x128', '5x3x9x7'])
def test_sync_bn_halves_merge_to_whole_batch_statistics(lib, ops, part, world):
    """tg_bn_local_stats per part -> tg_bn_merge_stats -> whole-batch statistics; tg_bn_lrelu_bwd_reduce per part,
    summed -> tg_bn_lrelu_bwd_apply -> whole-batch dx.  Part r is shifted by 0.7 r so the cross term of the merge
    carries most of the variance.

    k = per-part chain (as above) + world.  mean: gamma_{k+2} A.  invstd: with computed part means m_r and merged
    mean m, sum_r [sum (x - m_r)^2 + cnt_r (m_r - m)^2] differs from cnt var by sum_r cnt_r e_r^2 (e_r = m_r - mu_r,
    <= delta^2 cnt), by cnt_r sum (e_r - e)^2 (<= 4 delta^2 cnt) and, to first order, by 2 cnt_r sum (mu_r - mu)(e_r - e)
    (<= 4 delta D cnt, D = mean_r |mu_r - mu| from the data in float64):
      rel(var + eps) <= (5 delta^2 + 4 delta D) / var + gamma_k + 9 u;  invstd: half of it + 2 u.
    dx: as in the fused test with B_s0 = sum_r gamma_{k_r+1} sum_r |dz| + u |s0| (the host's fp32 sum of the parts)."""
    from tecogan_pytorch_amd.ops import _stream
    n, c, h, w = part
    hw, cnt_r = h * w, n * h * w
    cnt = cnt_r * world
    vec = hw % 4 == 0
    # tg_bn_local_stats / _bwd_reduce never slice: one block per channel, of bn_threads(n, hw) threads -- what the
    # geometry query reports while it does not slice this shape; otherwise the longer chain of the two block sizes
    threads, sl = R.bn_geometry(lib, n, c, hw)
    chain = lambda t: R.block_chain(R.bn_sweep_chain(n, hw, t, vec), t)
    k1 = chain(threads) if sl == 1 else max(chain(256), chain(1024))
    r = rs(world * 10 + n)
    xs = [f32(r.normal(0, 1, part) + 0.7 * i) for i in range(world)]
    x = torch.cat(xs)
    gamma, beta = f32(r.uniform(0.5, 1.5, c)), f32(r.normal(0, 0.5, c))
    dy = f32(r.normal(0, 1, x.shape))
    eps, mom, slope = 1e-5, 0.1, 0.2
    xd = x.cuda()
    gathered = torch.full((world, 2 * c), float('nan'), device='cuda')
    for i in range(world):
        assert lib.tg_bn_local_stats(xd[i * n:(i + 1) * n].data_ptr(), gathered[i].data_ptr(), n, c, hw, _stream()) == 0
    rm0, rv0 = f32(rs(3).normal(0, 1, c)), f32(rs(4).uniform(0.5, 2, c))
    rm, rv = rm0.cuda(), rv0.cuda()
    mean, invstd = torch.empty(c, device='cuda'), torch.empty(c, device='cuda')
    assert lib.tg_bn_merge_stats(gathered.data_ptr(), world, float(cnt_r), eps, mom, mean.data_ptr(), invstd.data_ptr(),
                                 rm.data_ptr(), rv.data_ptr(), c, _stream()) == 0
    yr, mr, vr, isr = R.bn_fwd_ref(x, gamma, beta, eps, slope)
    k = k1 + world
    xa = x.double().abs()
    b_mean = gk(k + 2) * xa.mean((0, 2, 3))
    delta = gk(k + 2) * xa.amax((0, 2, 3))
    mu_r = torch.stack([t.double().mean((0, 2, 3)) for t in xs])
    D = (mu_r - mr).abs().mean(0)
    rel_var = (5 * delta ** 2 + 4 * delta * D) / vr + gk(k) + 8 * U
    b_is_rel = 0.5 * (rel_var + U) + 2 * U
    tag = f'syncbn {part} x{world} k={k}'
    # the per-part (mean, M2) pairs themselves
    for i in range(world):
        m2r = ((xs[i].double() - mu_r[i].view(1, c, 1, 1)) ** 2).sum((0, 2, 3))
        ai, mx = xs[i].double().abs().mean((0, 2, 3)), xs[i].double().abs().amax((0, 2, 3))
        check(f'{tag} part {i} mean', gathered[i, :c], mu_r[i], gk(k1 + 1) * ai)
        check(f'{tag} part {i} M2', gathered[i, c:], m2r, cnt_r * (gk(k1 + 1) * mx) ** 2 + (gk(k1) + 3 * U) * m2r)
    check(f'{tag} mean', mean, mr, b_mean)
    check(f'{tag} invstd', invstd, isr, b_is_rel * isr)
    rmr, rvr = R.bn_running_ref(rm0, rv0, mr, vr, cnt, mom)
    m32 = float(np.float32(mom))
    check(f'{tag} running_mean', rm, rmr, 3 * U * ((1 - m32) * rm0.double()).abs() + m32 * b_mean + 2 * U * (m32 * mr).abs())
    check(f'{tag} running_var', rv, rvr, 3 * U * ((1 - m32) * rv0.double()).abs() + (rel_var + 4 * U) * m32 * vr * cnt / (cnt - 1.0))

    gd, bd, dyd = gamma.cuda(), beta.cuda(), dy.cuda()
    y = torch.full_like(xd, float('nan'))
    assert lib.tg_bn_lrelu_apply(xd.data_ptr(), mean.data_ptr(), invstd.data_ptr(), gd.data_ptr(), bd.data_ptr(), slope,
                                 y.data_ptr(), n * world, c, hw, _stream()) == 0
    sums = torch.full((world, 2 * c), float('nan'), device='cuda')
    for i in range(world):
        s_ = slice(i * n, (i + 1) * n)
        assert lib.tg_bn_lrelu_bwd_reduce(xd[s_].data_ptr(), y[s_].data_ptr(), dyd[s_].data_ptr(), mean.data_ptr(),
                                          invstd.data_ptr(), slope, sums[i].data_ptr(), n, c, hw, _stream()) == 0
    dxr, dgr, dbr, dz, xhat = R.bn_bwd_ref(x, y.cpu(), dy, gamma, mean.cpu(), invstd.cpu(), slope)
    b_s0 = gk(k1 + 1) * dz.abs().sum((0, 2, 3))
    b_s1 = gk(k1 + 4) * (dz * xhat).abs().sum((0, 2, 3))
    total = sums.cpu().double().sum(0).float()               # the all-reduce: one rounding of the exact sum of the parts
    check(f'{tag} sum dz', total[:c], dbr, b_s0 + U * dbr.abs())
    check(f'{tag} sum dz xhat', total[c:], dgr, b_s1 + U * dgr.abs())
    td = total.cuda()
    dx = torch.full_like(xd, float('nan'))
    assert lib.tg_bn_lrelu_bwd_apply(xd.data_ptr(), y.data_ptr(), dyd.data_ptr(), mean.data_ptr(), invstd.data_ptr(),
                                     gd.data_ptr(), td.data_ptr(), slope, 1.0 / cnt, dx.data_ptr(), n * world, c, hw,
                                     _stream()) == 0
    V = lambda t: t.double().view(1, c, 1, 1)
    gs = (V(gamma) * V(invstd.cpu())).abs()
    b_dx = gs * (V(b_s0 + U * dbr.abs()) + xhat.abs() * V(b_s1 + U * dgr.abs())) / cnt + \
        U * gs * (5 * dz.abs() + 6 * V(dbr).abs() / cnt + 8 * (xhat * V(dgr)).abs() / cnt)
    check(f'{tag} dx', dx, dxr, b_dx)


# =================================================================================================
# bias gradients: exact-sum data, bit-equal
# =================================================================================================
def bias_slice_starts(total, hw):
    """Offsets inside a plane at which the slices of a bias-gradient launch over `total` = images x hw elements
    start: ceil(total / 4096) slices (no case here reaches the launchers' block caps), each rounded up to a multiple of 4."""
    nslice = math.ceil(total / 4096)
    per = (math.ceil(total / nslice) + 3) & ~3
    return [(s * per) % hw for s in range(nslice) if s * per < total]


# mid = which of (bias_grad, bias_grad_multi, bias_grad_body) must have a slice that starts inside a plane
BIAS_CASES = [(40, 10, 11, (False, False, True)), (41, 10, 11, (True, True, True)), (75, 10, 11, (True, True, False)),
              (3, 50, 82, (True, True, True)), (5, 64, 64, (False, False, False)), (700, 2, 3, (False, True, True))]


def test_bias_cases_put_mid_plane_slices_on_every_form():
    """Each of the three launch forms meets several slices with a mid-plane start on the scalar path (hw % 4 != 0) and
    on the 16-byte path (hw % 4 == 0, start % 4 == 0)."""
    for form in range(3):
        kinds = {(h * w) % 4 == 0 for n, h, w, mid in BIAS_CASES if mid[form]}
        assert kinds == {False, True}, form


@pytest.mark.parametrize('n,h,w,mid', BIAS_CASES, ids=[f'{n}x{h * w}' for n, h, w, _ in BIAS_CASES])
def test_bias_grads_exact(ops, n, h, w, mid):
    """ops.bias_grad (n images) / bias_grad_multi (3 segments of n) / bias_grad_body (2 frames of n x 3 layers) on
    values j / 8: every slice's partial and every atomic add is exact, so db must be the fp32 image of the float64
    sum -- a slice that starts at the wrong offset of a plane, or a dropped / doubled 16-byte group, cannot hide.
    Each form cuts its own total (n hw, 3 n hw, 2 n hw) into slices and has its own copy of the plane walk, so the
    slice starts are computed, and asserted, per form: hw = 110 and hw = 6 are the scalar path, hw = 4100 the 16-byte
    path with mid-plane starts, hw = 4096 slices on plane boundaries.  (The issue's hw = 110, n = 40 puts the single
    and multi forms' boundaries on plane starts; n = 41 and 75 are added for them.)"""
    c, hw = 5, h * w
    assert 3 * n * hw * 8 <= 2 ** 24
    for form, images in (('bias_grad', n), ('bias_grad_multi', 3 * n), ('bias_grad_body', 2 * n)):
        st = bias_slice_starts(images * hw, hw)
        print(f'[measured] {form} n={n} hw={hw}: {len(st)} slices, start offsets in plane {st}')
        assert len(st) > 1
        assert any(st) == mid[('bias_grad', 'bias_grad_multi', 'bias_grad_body').index(form)], (form, st)
    dy = R.exact_values(n + hw, (n, c, h, w))
    want = dy.double().sum((0, 2, 3))
    db0 = R.exact_values(3, (c,)) * 8
    dyd = dy.cuda()
    db = torch.full((c,), 7.0, device='cuda')
    ops.bias_grad(dyd, db, accumulate=False)
    bits_equal(f'bias_grad {n}x{hw} overwrite', db, want)
    db = db0.cuda()
    ops.bias_grad(dyd, db, accumulate=True)
    bits_equal(f'bias_grad {n}x{hw} accumulate', db, db0.double() + want)
    segs = [R.exact_values(100 + i + n, (n, c, h, w)) for i in range(3)]
    want3 = sum(s.double().sum((0, 2, 3)) for s in segs)
    sd = [s.cuda() for s in segs]
    db = torch.full((c,), 7.0, device='cuda')
    ops.bias_grad_multi(sd, db, accumulate=False)
    bits_equal(f'bias_grad_multi {n}x{hw} overwrite', db, want3)
    db = db0.cuda()
    ops.bias_grad_multi(sd, db, accumulate=True)
    bits_equal(f'bias_grad_multi {n}x{hw} accumulate', db, db0.double() + want3)
    # body form: frames of (layers, n, c, h, w); dbs[L] accumulates layer L over all frames
    frames = [R.exact_values(200 + i + n, (3, n, c, h, w)) for i in range(2)]
    dbs0 = [R.exact_values(300 + L, (c,)) * 8 for L in range(3)]
    dbs = [t.cuda() for t in dbs0]
    ops.bias_grad_body([f.cuda() for f in frames], dbs)
    for L in range(3):
        bits_equal(f'bias_grad_body {n}x{hw} layer {L}', dbs[L],
                   dbs0[L].double() + sum(f[L].double().sum((0, 2, 3)) for f in frames))


# =================================================================================================
# loss reductions
# =================================================================================================
def loss_chain(n, cap):
    """grid_for(n, cap) blocks of 256: elements per thread + 6 shuffles + 4 waves + one atomic add per block."""
    grid = min(cap, max(1, math.ceil(n / 256)))
    return math.ceil(n / (grid * 256)) + 6 + 4 + grid


@pytest.mark.parametrize('n', [N_BIG, N_SMALL])
def test_charbonnier(ops, n):
    """r = sqrt(d^2 + eps), d = fl(x - y) (u |d| <= u r).  rel(r) <= 1/2 (2 u + u + u) + E_SQRT u = (2 + E_SQRT) u
    (d twice in the square, the product, the add; halved by the root).  loss = scale * sum r:
    (gamma_k + (3 + E_SQRT) u) scale sum r (one more u for the partial * scale), k from grid_for(n, 1024).
    dx = gscale d / r: d (1 u), r, gscale * d (1 u), the division: (4 + E_SQRT + E_DIV) u |dx|."""
    r_ = rs(n)
    x, y = f32(r_.uniform(-1, 1, n)), f32(r_.uniform(-1, 1, n))
    y[:5] = x[:5]                                              # d == 0: r = sqrt(eps), dx = 0
    eps, scale, gscale = 1e-6, 0.37, 1.7
    acc = torch.zeros(1, device='cuda')
    dx = ops.charbonnier(x.cuda(), y.cuda(), acc, scale, grad_scale=gscale, eps=eps)
    terms, g = R.charbonnier_ref(x, y, float(np.float32(eps)))
    k = loss_chain(n, 1024)
    s32, g32 = float(np.float32(scale)), float(np.float32(gscale))
    check(f'charbonnier n={n} k={k} loss', acc, s32 * terms.sum(), (gk(k) + (3 + E_SQRT) * U) * s32 * terms.sum())
    check(f'charbonnier n={n} dx', dx, g32 * g, (4 + E_SQRT + E_DIV) * U * (g32 * g).abs())
    assert (dx[:5] == 0).all()


@pytest.mark.parametrize('n', [N_BIG, N_SMALL])
@pytest.mark.parametrize('mode', [1, 2], ids=['l1', 'mse'])
def test_pixel_loss(ops, n, mode):
    """Generic: term |d| or d^2 with d = fl(x - y): (gamma_k + 2 | 4 u) scale sum terms (d, [square 2 u + u], partial *
    scale), k from grid_for(n, 1024); dx: L1 sign(d) gscale exactly (0 at d == 0), MSE gscale * 2 * d: 3 u.
    Exact-sum: x in j / 2 (|j| <= 2), y in j / 2 (|j| <= 1): |d| <= 1.5 in halves, d^2 <= 2.25 in quarters, n * 9 < 2^24,
    power-of-two scales: loss and gradient bit-equal."""
    r_ = rs(n + mode)
    x, y = f32(r_.uniform(-1, 1, n)), f32(r_.uniform(-1, 1, n))
    y[:5] = x[:5]
    scale, gscale = 0.37, 1.7
    s32, g32 = float(np.float32(scale)), float(np.float32(gscale))
    acc = torch.zeros(1, device='cuda')
    dx = ops.pixel_loss(x.cuda(), y.cuda(), mode, acc, scale, grad_scale=gscale)
    terms, g = R.pixel_ref(x, y, mode)
    k = loss_chain(n, 1024)
    check(f'pixel_loss mode={mode} n={n} k={k} loss', acc, s32 * terms.sum(), (gk(k) + (2 if mode == 1 else 4) * U) * s32 * terms.sum())
    if mode == 1:
        bits_equal(f'pixel_loss l1 n={n} dx', dx, g32 * g)
        assert (dx[:5] == 0).all()
    else:
        check(f'pixel_loss mse n={n} dx', dx, g32 * g, 3 * U * (g32 * g).abs())
    assert n * 9 < 2 ** 24
    xe, ye = R.exact_values(n, (n,), 2, 2), R.exact_values(n + 1, (n,), 2, 1)
    acc = torch.full((1,), 3.0, device='cuda')
    dx = ops.pixel_loss(xe.cuda(), ye.cuda(), mode, acc, 2.0 ** -10, grad_scale=0.25)
    terms, g = R.pixel_ref(xe, ye, mode)
    bits_equal(f'pixel_loss mode={mode} n={n} loss (exact)', acc, 3.0 + 2.0 ** -10 * terms.sum().view(1))
    bits_equal(f'pixel_loss mode={mode} n={n} dx (exact)', dx, 0.25 * g)


@pytest.mark.parametrize('n', [N_BIG, N_SMALL])
@pytest.mark.parametrize('lsgan', [False, True], ids=['vanilla', 'lsgan'])
@pytest.mark.parametrize('target', [1.0, 0.0])
def test_bce_logits(ops, n, lsgan, target):
    """stats = scale * (sum loss, sum x, sum log(sigmoid(x) + 1e-8)), dx = gscale * dloss/dx; NaN-prefilled dx_out.
    With w = exp(-|x|), sig = 1 / (1 + exp(-x)): rel(sig) <= e_sig u, e_sig = E_EXP + 1 + E_DIV (exp's error reaches sig
    scaled by exp(-x) sig <= 1; the add; the division).
      vanilla term max(x,0) - x t + log1p(w): u (E_EXP w [d log1p = dw / (1 + w)] + E_LOG1P log1p(w) + |x t|
               + 2 (max(x,0) + |x t| + log1p(w)))   (the two additions at most double-count every operand)
      lsgan term (x - t)^2: 3 u;   sum x: exact terms;   log(sig + 1e-8): arg within (e_sig + 1) u relatively, so
               (e_sig + 1) u + E_LOG u |log|.  logf is accurate to E_LOG u of its RESULT; near arg = 1 (x >> 0) the
               result -> 0 and the (e_sig + 1) u absolute term carries the bound.
      every sum: + (gamma_k + u) sum |term| (k from grid_for(n, 256); partial * scale).
      dx vanilla gscale (sig - t): gscale (e_sig u sig + 2 u |sig - t|) + FLT_MIN (x = 90: exp overflows, sig = 0
               against 8e-40); lsgan gscale * 2 (x - t): 3 u.
    Logits +-30 and +-90 are planted: every output finite.  Exact-sum inputs (x in j / 2, |j| <= 1, power-of-two
    scales): sum x and the LSGAN loss and gradient bit-equal."""
    r_ = rs(n + int(target))
    x = f32(r_.normal(0, 3, n))
    x[:4] = torch.tensor([30.0, -30.0, 90.0, -90.0])
    scale, gscale = 0.37, 1.7
    s32, g32 = float(np.float32(scale)), float(np.float32(gscale))
    stats = torch.zeros(3, device='cuda')
    dx_out = torch.full((n,), float('nan'), device='cuda')
    dx = ops.bce_logits(x.cuda(), target, stats, scale, grad_scale=gscale, dx_out=dx_out, lsgan=lsgan)
    assert dx.data_ptr() == dx_out.data_ptr()
    t0, t1, t2, g = R.bce_ref(x, target, lsgan)
    k = loss_chain(n, 256)
    xd = x.double()
    sig = 1.0 / (1.0 + torch.exp(-xd))
    e_sig = E_EXP + 1 + E_DIV
    wv = torch.exp(-xd.abs()); l1p = torch.log1p(wv)
    if lsgan:
        tb0 = 3 * U * t0
    else:
        tb0 = U * (E_EXP * wv + E_LOG1P * l1p + (xd * target).abs() + 2 * (xd.clamp_min(0) + (xd * target).abs() + l1p))
    tb2 = (e_sig + 1) * U + E_LOG * U * t2.abs()
    tag = f'bce lsgan={lsgan} t={target} n={n} k={k}'
    check(f'{tag} loss', stats[0], s32 * t0.sum(), s32 * (tb0.sum() + (gk(k) + U) * t0.abs().sum()))
    check(f'{tag} sum x', stats[1], s32 * t1.sum(), s32 * (gk(k) + U) * t1.abs().sum())
    check(f'{tag} sum log sig', stats[2], s32 * t2.sum(), s32 * (tb2.sum() + (gk(k) + U) * t2.abs().sum()))
    if lsgan:
        check(f'{tag} dx', dx, g32 * g, 3 * U * (g32 * g).abs())
    else:
        check(f'{tag} dx', dx, g32 * g, g32 * (e_sig * U * sig + 2 * U * (sig - target).abs()) + FLT_MIN)
    # the four planted logits against the fp64 formula itself
    print(f'[measured] {tag} planted logits dx {dx[:4].tolist()}')
    assert torch.isfinite(dx[:4]).all() and torch.isfinite(stats).all()

    xe = R.exact_values(n, (n,), 2, 1)
    assert n * 9 < 2 ** 24
    stats = torch.zeros(3, device='cuda')
    dx = ops.bce_logits(xe.cuda(), target, stats, 2.0 ** -10, grad_scale=0.25, lsgan=lsgan)
    t0, t1, _, g = R.bce_ref(xe, target, lsgan)
    bits_equal(f'{tag} sum x (exact)', stats[1:2], 2.0 ** -10 * t1.sum().view(1))
    if lsgan:
        bits_equal(f'{tag} loss (exact)', stats[0:1], 2.0 ** -10 * t0.sum().view(1))
        bits_equal(f'{tag} dx (exact)', dx, 0.25 * g)


def test_bce_extreme_logits_match_the_fp64_formula(ops):
    """x = +-30, +-90 alone (n = 4, one block, k = 1 + 6 + 4 + 1): the statistics are finite and equal the float64
    formula evaluated with the same + 1e-8 under test_bce_logits' term bounds."""
    x = torch.tensor([30.0, -30.0, 90.0, -90.0])
    for target in (1.0, 0.0):
        stats = torch.zeros(3, device='cuda')
        dx = ops.bce_logits(x.cuda(), target, stats, 1.0, grad_scale=1.0)
        t0, t1, t2, g = R.bce_ref(x, target)
        xd = x.double()
        sig = 1.0 / (1.0 + torch.exp(-xd)); wv = torch.exp(-xd.abs()); l1p = torch.log1p(wv)
        e_sig = E_EXP + 1 + E_DIV
        tb0 = U * (E_EXP * wv + E_LOG1P * l1p + (xd * target).abs() + 2 * (xd.clamp_min(0) + (xd * target).abs() + l1p))
        tb2 = (e_sig + 1) * U + E_LOG * U * t2.abs()
        k = 12
        check(f'bce extreme t={target} loss', stats[0], t0.sum(), tb0.sum() + gk(k) * t0.abs().sum())
        check(f'bce extreme t={target} sum x', stats[1], t1.sum(), gk(k) * t1.abs().sum())
        check(f'bce extreme t={target} sum log sig', stats[2], t2.sum(), tb2.sum() + gk(k) * t2.abs().sum())
        check(f'bce extreme t={target} dx', dx, g, e_sig * U * sig + 2 * U * (sig - target).abs() + FLT_MIN)


@pytest.mark.parametrize('shape', [(7, 3, 149907, 1), (1, 3, N_SMALL, 1)], ids=['big', 'small'])
def test_cosine_loss(ops, shape):
    """Per pixel, c channels, relative to |a| |b| (clamped norms nac, nbc): dot within gamma_{c+1} sum |a_c b_c| <=
    gamma_{c+1} nac nbc (products + c adds); each norm rel 1/2 gamma_{c+1} + E_SQRT u; nac * nbc, 1 / ., dot * inv:
    (2 + E_DIV) u.  B_cs = gamma_{c+1} + |cs| e_n, e_n = gamma_{c+1} + (2 E_SQRT + E_DIV + 2) u.
    term 1 - cs: B_cs + u |1 - cs|; loss: scale (sum term bounds + (gamma_k + u) sum |1 - cs|), k from grid_for(npix, 2048).
    da_c = -gscale (b_c inv - k_ a_c), k_ = cs / nac^2 (0 when |a| <= eps):
      |b_c inv| (e_n + u) + |a_c| / nac^2 B_cs + |k_ a_c| (e_n + 3 u) + u (|b_c inv| + |k_ a_c|), then + u |da| for gscale.
    Pixels with |a| < eps and all-zero pixels are planted: no gradient through the clamped norm (da = -gscale b / (eps |b|))."""
    n, c, h, w = shape
    r_ = rs(n + h)
    a, b = f32(r_.normal(0, 1, shape)), f32(r_.normal(0, 1, shape))
    a[0, :, 0, 0] = 1e-10
    a[0, :, 1, 0] = 0.0
    a[-1, :, -1, 0] = 3e-9
    eps, scale, gscale = 1e-8, 0.37, 1.7
    s32, g32, e32 = float(np.float32(scale)), float(np.float32(gscale)), float(np.float32(eps))
    acc = torch.zeros(1, device='cuda')
    da = ops.cosine_loss(a.cuda(), b.cuda(), acc, scale, grad_scale=gscale, eps=eps)
    terms, g = R.cosine_ref(a, b, e32)
    ad, bd_ = a.double(), b.double()
    nac = ad.norm(dim=1, keepdim=True).clamp_min(e32); nbc = bd_.norm(dim=1, keepdim=True).clamp_min(e32)
    cs = 1.0 - terms.unsqueeze(1)
    e_n = gk(c + 1) + (2 * E_SQRT + E_DIV + 2) * U
    b_cs = gk(c + 1) + cs.abs() * e_n
    k = loss_chain(n * h * w, 2048)
    tb = (b_cs + U * (1 - cs).abs()).sum()
    check(f'cosine {shape} k={k} loss', acc, s32 * terms.sum(), s32 * (tb + (gk(k) + U) * terms.abs().sum()))
    inv = 1.0 / (nac * nbc)
    k_ = torch.where(ad.norm(dim=1, keepdim=True) > e32, cs / (nac * nac), torch.zeros_like(cs))
    t1, t2 = (bd_ * inv).abs(), (k_ * ad).abs()
    b_da = g32 * (t1 * (e_n + U) + ad.abs() / (nac * nac) * b_cs + t2 * (e_n + 3 * U) + U * (t1 + t2)) + U * (g32 * g).abs()
    check(f'cosine {shape} da', da, g32 * g, b_da)
    want0 = -g32 * bd_[0, :, 1, 0] / (e32 * bd_[0, :, 1, 0].norm())
    assert torch.allclose(da[0, :, 1, 0].cpu().double(), want0, rtol=1e-5, atol=0)


# =================================================================================================
# element-wise kernels past the grid cap
# =================================================================================================
@pytest.mark.parametrize('act', [1, 2, 3], ids=['relu', 'lrelu', 'tanh24'])
def test_act_bwd_past_the_cap(ops, act):
    """relu / lrelu: one IEEE product at most: bit-equal to fp32(float64) (0.2f is the fp32 constant).
    tanh24: g (24 - o o / 24): |g| (3 u o^2 / 24 [o o, 1/24 rounded, product] + u |24 - o^2/24|) + u |r|."""
    r_ = rs(act)
    dy = f32(r_.normal(0, 1, N_BIG))
    y = f32(r_.uniform(-24, 24, N_BIG))
    y[:3] = torch.tensor([0.0, -0.0, 24.0])
    out = torch.full((N_BIG,), float('nan'), device='cuda')
    ops.act_bwd(dy.cuda(), y.cuda(), act, out=out)
    g, o = dy.double(), y.double()
    if act == 1:
        bits_equal('act_bwd relu', out, torch.where(o > 0, g, torch.zeros_like(g)))
    elif act == 2:
        bits_equal('act_bwd lrelu', out, torch.where(o > 0, g, g * float(np.float32(0.2))))
    else:
        ref = g * (24.0 - o * o / 24.0)
        check('act_bwd tanh24', out, ref, g.abs() * (3 * U * o * o / 24 + U * (24 - o * o / 24).abs()) + U * ref.abs())


def test_axpy_div_scalar_channel_norm_past_the_cap(ops):
    """axpy_ on exact data (j / 8, a = 0.5: product and sum exact): bit-equal.  div_scalar_: one IEEE division,
    bit-equal to fp32(float64 quotient) (double rounding is innocuous for a quotient at 53 >= 2 * 24 + 2 bits).
    channel_norm: fl(fl(x - m) / s): u |x - m| / |s| for the subtraction + u |y| for the division; without a mean
    the single division is bit-equal."""
    y0, x = R.exact_values(1, (N_BIG,)), R.exact_values(2, (N_BIG,))
    yd = y0.cuda()
    ops.axpy_(yd, x.cuda(), 0.5)
    bits_equal('axpy_', yd, y0.double() + 0.5 * x.double())
    v = f32(rs(3).normal(0, 10, N_BIG))
    out = torch.full((N_BIG,), float('nan'), device='cuda')
    ops.div_scalar_(out, 3.0, x=v.cuda())
    bits_equal('div_scalar_ / 3', out, v.double() / 3.0)
    vd = v.cuda()
    ops.div_scalar_(vd, 7.0)
    bits_equal('div_scalar_ / 7 in place', vd, v.double() / 7.0)
    c, hw = 3, 349785
    assert c * hw > R.GRID_CAP_THREADS
    xx = f32(rs(4).uniform(0, 1, (1, c, hw, 1)))
    mean, std = f32([0.485, 0.456, 0.406]), f32([0.229, 0.224, 0.225])
    got = ops.channel_norm(xx.cuda(), mean.cuda(), std.cuda())
    m, s = mean.double().view(1, c, 1, 1), std.double().view(1, c, 1, 1)
    ref = (xx.double() - m) / s
    check('channel_norm', got, ref, (1 + 2 * U) * (U * (xx.double() - m).abs() / s + U * ref.abs()))   # (u^2 terms)
    got = ops.channel_norm(xx.cuda(), None, std.cuda())
    bits_equal('channel_norm, no mean', got, xx.double() / s)


def test_maxpool2_bwd_ties_past_the_cap(ops):
    """x takes four values only, so most windows hold ties: the gradient goes to the FIRST maximum in row-major
    window order (as torch's CPU max_pool2d), everything else -- the odd last row and column included -- is 0."""
    n, c, h, w = 1, 3, 591, 593
    assert n * c * h * w > R.GRID_CAP_THREADS
    x = rs(1).randint(0, 4, (n, c, h, w)).astype(np.float32)
    g = rs(2).normal(0, 1, (n, c, h // 2, w // 2)).astype(np.float32)
    win = x[:, :, :h // 2 * 2, :w // 2 * 2].reshape(n, c, h // 2, 2, w // 2, 2).transpose(0, 1, 2, 4, 3, 5).reshape(n, c, h // 2, w // 2, 4)
    arg = win.argmax(-1)                                       # first maximum
    ref = np.zeros((n, c, h // 2, 2, w // 2, 2), np.float32)
    for a in range(4):
        ref[:, :, :, a // 2, :, a % 2] = np.where(arg == a, g, 0)
    full = np.zeros_like(x)
    full[:, :, :h // 2 * 2, :w // 2 * 2] = ref.reshape(n, c, h // 2 * 2, w // 2 * 2)
    got = ops.maxpool2_bwd(f32(x).cuda(), f32(g).cuda())
    assert torch.equal(got.cpu(), f32(full))
    xt = f32(x).requires_grad_(True)
    F.max_pool2d(xt, 2, 2).backward(f32(g))
    assert torch.equal(xt.grad, f32(full))                     # torch CPU agrees on the tie rule


@pytest.mark.parametrize('deg', ['BD', 'BI'])
def test_upsample_bwd_past_the_cap(ops, deg):
    """Transpose of the x2 up-sampler (grid cap 8192 blocks) against float64 autograd of the oracle's forward.
    Each dx sums at most (4 s)^2 = 64 products w g, |w| <= 1.375^2 < 1.9 (the bicubic taps of one phase sum to 1.375
    in magnitude, and clamped border taps add up on one input; bilinear: 1):
    gamma_{64 + 3} * 1.9 * mul * (sum of |g| over the (4 s)^2 outputs that can reach the input) (+3: weight products, mul)."""
    s, n, c, h, w = 2, 1, 3, 701, 1000
    assert n * c * h * w > 8192 * 256
    g = f32(rs(5).normal(0, 1, (n, c, h * s, w * s)))
    x = torch.zeros(n, c, h, w, dtype=torch.float64, requires_grad=True)
    (float(s) * O.upsample(x, s, deg)).backward(g.double())
    got = ops.upsample_bwd(g.cuda(), s, ops.UP_MODE[deg], mul=float(s))
    win = F.avg_pool2d(F.pad(g.double().abs(), (2 * s, 2 * s, 2 * s, 2 * s)), 4 * s, stride=s)[:, :, :h, :w] * (4 * s) ** 2
    check(f'upsample_bwd {deg}', got, x.grad, gk(67) * 1.9 * s * win)


def test_depth_to_space_past_the_cap(ops):
    """A permutation: exact.  Scalar form (w % 4 != 0) past its cap of 8192 blocks, 16-byte forms (s = 2, 4) below."""
    for (n, c, h, w, s) in [(1, 3, 419, 421, 2), (2, 3, 64, 128, 2), (1, 2, 33, 64, 4)]:
        x = f32(rs(s).normal(0, 1, (n, s * s * c, h, w)))
        if w % 4:
            assert n * c * h * s * w * s > 8192 * 256
        ref = x.view(n, s, s, c, h, w).permute(0, 3, 4, 1, 5, 2).reshape(n, c, h * s, w * s)
        got = ops.depth_to_space(x.cuda(), s)
        assert torch.equal(got.cpu(), ref), (n, c, h, w, s)


@pytest.mark.parametrize('pad', [0, 1])
def test_downsample_bd_past_the_cap(ops, pad):
    """7 x 7 blur + stride-2 decimation, valid and reflect-padded, > 4096 * 256 outputs, against float64 conv2d:
    49 products and adds: gamma_{50} * (|k| conv |x|)."""
    ks, s, c, h, w = 7, 2, 3, 1203, 1200
    kern = rs(1).uniform(0, 1, (ks, ks)).astype(np.float32)
    kern[0, 0] += 0.123 + pad                                   # (ops caches the device copy by size and centre tap)
    kern[ks // 2, ks // 2] = 1.0 + pad
    x = f32(rs(2).normal(0, 1, (1, c, h, w)))
    got = ops.downsample_bd(x.cuda(), kern, s, pad)
    assert got.numel() > R.GRID_CAP_THREADS
    xd = x.double()
    if pad:
        xd = F.pad(xd, (3, 3, 3, 3), mode='reflect')
    kd = torch.from_numpy(kern).double().view(1, 1, ks, ks).expand(c, 1, ks, ks)
    ref = F.conv2d(xd, kd, stride=s, groups=c)
    assert ref.shape == got.shape
    check(f'downsample_bd pad={pad}', got, ref, gk(50) * F.conv2d(xd.abs(), kd.abs(), stride=s, groups=c))


def test_linear1_bwd_past_the_cap(ops):
    """rows = 3, k past the cap.  dx = fl(dy_r w): bit-equal.  dw += sum_r dy_r x_r: gamma_{rows + 2} sum |dy x| + u |dw|
    (products, adds, the accumulation onto the start value); db likewise."""
    rows, k = 3, N_BIG
    r_ = rs(9)
    x, wt, dy = f32(r_.normal(0, 1, (rows, k))), f32(r_.normal(0, 1, k)), f32(r_.normal(0, 1, (rows, 1)))
    dw0, db0 = f32(r_.normal(0, 1, k)), f32([0.75])
    dw, db = dw0.cuda(), db0.cuda()
    dx = ops.linear1_bwd(x.cuda(), wt.cuda(), dy.cuda(), dw=dw, db=db, need_dx=True)
    bits_equal('linear1_bwd dx', dx, dy.double() * wt.double().view(1, k))
    ref = dw0.double() + (dy.double() * x.double()).sum(0)
    check('linear1_bwd dw', dw, ref, gk(rows + 2) * (dy.double() * x.double()).abs().sum(0) + U * ref.abs() + U * dw0.double().abs())
    check('linear1_bwd db', db, db0.double() + dy.double().sum(), gk(rows + 1) * dy.double().abs().sum() + U)


@pytest.mark.parametrize('step', [1, 1000])
def test_adam_step_past_the_cap(ops, step):
    """torch.optim.Adam with weight_decay != 0, float64 from the fp32 hyper-parameters.  g' = g + wd p (2 u);
    m' = b1 m + (1 - b1) g': 2 u |b1 m| + (4 + 2) u |(1 - b1) g'| ((1 - b1) rounded, product, add; g' carries 2 u);
    v' = b2 v + (1 - b2) g'^2: 2 u |b2 v| + (4 + 5) u (1 - b2) g'^2;
    upd = (lr / bc1) m' / (sqrt(v') / sbc2 + eps): bc1, sbc2 from the host's powf / sqrtf (4 u each allowed), so
    rel(upd) <= B_m / |m'| + 1/2 B_v / v' + (E_SQRT + 2 E_DIV + 4 + 8) u;  p' = p - upd: B_upd + u |p'|.
    The guarded form with a non-zero slot leaves p, m, v untouched (bit for bit)."""
    n = N_BIG
    r_ = rs(step)
    p, g = f32(r_.normal(0, 1, n)), f32(r_.normal(0, 0.1, n))
    m, v = f32(r_.normal(0, 0.1, n)), f32(r_.uniform(1e-4, 1e-2, n))
    lr, b1, b2, eps, wd = 1e-3, 0.9, 0.999, 1e-8, 0.01
    pd, md, vd, gd = p.cuda(), m.cuda(), v.cuda(), g.cuda()
    slot = torch.ones(1, device='cuda')
    ops.adam_step(pd, gd, md, vd, lr, (b1, b2), eps, wd, step, skip=slot)
    assert torch.equal(pd.cpu(), p) and torch.equal(md.cpu(), m) and torch.equal(vd.cpu(), v)
    slot.zero_()
    ops.adam_step(pd, gd, md, vd, lr, (b1, b2), eps, wd, step, skip=slot)
    pr, mr, vr = R.adam_ref(p, g, m, v, lr, b1, b2, eps, wd, step)
    f = lambda s_: float(np.float32(s_))
    gp = g.double() + f(wd) * p.double()
    b_gp = 2 * U * (g.double().abs() + (f(wd) * p.double()).abs())
    b_m = 2 * U * (f(b1) * m.double()).abs() + (1 - f(b1)) * (b_gp + 4 * U * gp.abs())
    b_v = 2 * U * f(b2) * v.double() + (1 - f(b2)) * (2 * gp.abs() * b_gp + 5 * U * gp * gp)
    check(f'adam step={step} m', md, mr, b_m)
    check(f'adam step={step} v', vd, vr, b_v)
    denom = torch.sqrt(vr) / math.sqrt(1 - f(b2) ** step) + f(eps)
    upd = (f(lr) / (1 - f(b1) ** step)) * mr / denom
    b_upd = (f(lr) / (1 - f(b1) ** step)) / denom * b_m + upd.abs() * (0.5 * b_v / vr + (E_SQRT + 2 * E_DIV + 12) * U)
    check(f'adam step={step} p', pd, pr, (1 + 2 * U) * (b_upd + U * (pr.abs() + b_upd)))              # (fl(p - upd): u |computed p'|)
    # the unguarded entry computes the same thing
    p2, m2, v2 = p.cuda(), m.cuda(), v.cuda()
    ops.adam_step(p2, gd, m2, v2, lr, (b1, b2), eps, wd, step)
    assert torch.equal(p2, pd) and torch.equal(m2, md) and torch.equal(v2, vd)
