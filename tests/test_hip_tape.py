"""Every node type of models/train_graph.py, and the branches of its gradient bookkeeping, against CPU float64
autograd of the same one-to-three-node graph.

Each case builds its graph twice through `Twin` -- on the tape (device, fp32) and in torch autograd (CPU, float64) --
seeds the output gradient with tape.add_grad, runs tape.backward() and compares every input gradient and every
parameter gradient, bias included.  ReLU / LeakyReLU decisions of the reference are taken from the device's forward
output (tape_ref.act_ref) and the largest pre-activation decided the other way must lie within the forward tolerance,
so pinning cannot hide a wrong forward pass; kinked ops fed from leaves get kink-free inputs (tape_ref.kinkfree_flow,
distinct_windows).

Tolerances: max |got - ref| / max |ref| <= 2e-5 for gradients (tests/test_hip_train_ops.py: "different summation order
only"), 1e-5 for forward outputs (2e-6 for linear1, the number of test_linear1_forward_long_rows against float64).
A node that picks a branch by shape is given the smallest shape that takes each branch; the library's own predicates
are asked for the shape and a counting wrapper around the `ops` function shows the branch ran."""
import collections

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import tecogan_oracle as O
from tests import tape_ref as TR

TOL, FWD_TOL = 2e-5, 1e-5
NONE, RELU, LRELU, TANH24 = 0, 1, 2, 3
V = collections.namedtuple('V', 'd r')          # one tensor: on the device (fp32) / in the float64 autograd graph


@pytest.fixture(scope='module')
def ops():
    import tecogan_pytorch_amd.ops as ops_
    return ops_


@pytest.fixture(scope='module')
def TG(ops):
    from tecogan_pytorch_amd.models import train_graph
    assert (train_graph.NONE, train_graph.RELU, train_graph.LRELU, train_graph.TANH24) == (NONE, RELU, LRELU, TANH24)
    return train_graph


def rs(seed, shape, lo=-1.0, hi=1.0):
    return torch.from_numpy(np.random.RandomState(seed).uniform(lo, hi, shape).astype(np.float32))


def relerr(a, b):
    a = a.detach().cpu().double(); b = b.detach().cpu().double()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def conv(cin, cout, seed, transposed=False, frozen=False):
    from tecogan_pytorch_amd.models.networks.tecogan_nets import _Conv
    torch.manual_seed(seed)
    m = _Conv(cin, cout, transposed=transposed).cuda()
    if frozen:
        m.requires_grad_(False)
    return m


def conv4(ci, co, seed, frozen=False):
    from tecogan_pytorch_amd.models.networks.tecogan_nets import _Conv4
    torch.manual_seed(seed)
    m = _Conv4(ci, co).cuda()
    if frozen:
        m.requires_grad_(False)
    return m


def counting(monkeypatch, ops, *names):
    """Wraps ops.<name>: returns {name: [(args, kwargs), ...]} filled as the tape calls them."""
    calls = {n: [] for n in names}
    for name in names:
        fn = getattr(ops, name)

        def wrap(*a, _fn=fn, _name=name, **k):
            calls[_name].append((a, k))
            return _fn(*a, **k)
        monkeypatch.setattr(ops, name, wrap)
    return calls


class Twin:
    """One graph twice: tape nodes on the device, torch float64 autograd on the CPU."""

    def __init__(self, TG):
        self.TG, self.tape, self.loss, self.params = TG, TG.Tape(), 0.0, {}

    def leaf(self, t, grad=True):
        return V(t.cuda().contiguous(), t.double().requires_grad_(grad))

    def p(self, prm):
        if prm is None:
            return None
        ent = self.params.get(id(prm))
        if ent is None:
            assert prm.grad is None
            ent = self.params[id(prm)] = (prm, prm.detach().cpu().double().requires_grad_(prm.requires_grad))
        return ent[1]

    def out(self, name, yd, z64, act=NONE, tol=FWD_TOL):
        y64, slack = TR.act_ref(z64, yd, act)
        scale = y64.detach().abs().max().item()
        e = (yd.detach().cpu().double() - y64.detach()).abs().max().item()
        print(f'[measured] forward {name}: err {e:.3e} slack {slack:.3e} allowed {tol * scale:.3e}')
        assert yd.shape == y64.shape and e <= tol * scale and slack <= tol * scale, (name, e, slack, tol * scale)
        return V(yd, y64)

    def seed(self, v, seed, mul=1.0):
        dy = rs(seed, v.d.shape) * mul
        self.tape.add_grad(v.d, dy.cuda())
        self.loss = self.loss + (v.r * dy.double()).sum()

    def backward(self):
        self.tape.backward()
        self.loss.backward()
        t = self.tape
        assert not t.deferred and not t.deferred_bias and not t.deferred_body and not t.nodes

    def check(self, name, v, tol=TOL):
        got = self.tape.grad(v.d)
        assert got is not None and v.r.grad is not None, name
        e = relerr(got, v.r.grad)
        print(f'[measured] grad {name}: relerr {e:.3e}')
        assert got.shape == v.r.grad.shape and e <= tol, (name, e)

    def check_none(self, v):
        assert self.tape.grad(v.d) is None and v.r.grad is None

    def check_params(self, tol=TOL):
        assert self.params
        for prm, r in self.params.values():
            if not prm.requires_grad:
                assert prm.grad is None and r.grad is None          # frozen: no buffer is created
                continue
            e = relerr(prm.grad, r.grad)
            print(f'[measured] grad parameter {tuple(prm.shape)}: relerr {e:.3e}')
            assert e <= tol, (tuple(prm.shape), e)

    # ---- nodes ------------------------------------------------------------------------------------
    def conv3x3(self, layer, x, act=NONE, x2=None, res=None, **kw):
        yd = self.TG.conv3x3(self.tape, layer, x.d, act, x2=None if x2 is None else x2.d,
                             res=None if res is None else res.d, **kw)
        xin = x.r if x2 is None else torch.cat([x.r, x2.r], 1)
        z = F.conv2d(xin, self.p(layer.weight), self.p(layer.bias), padding=1)
        return self.out('conv3x3', yd, z if res is None else z + res.r, act)

    def conv3x3_small(self, layer, x, act=NONE, up_src=None, deg=None, up_scale=1, res=None):
        ops = self.TG.ops
        yd = self.TG.conv3x3_small(self.tape, layer, x.d, act, up_src=None if up_src is None else up_src.d,
                                   up_mode=ops.UP_MODE[deg] if deg else ops.UP_NONE, up_scale=up_scale,
                                   res=None if res is None else res.d)
        z, _ = TR.act_ref(F.conv2d(x.r, self.p(layer.weight), self.p(layer.bias), padding=1), yd, act)
        assert act in (NONE, TANH24)                    # (smooth: the residual forms add to the ACTIVATED conv)
        if up_src is not None:
            z = z + O.upsample(up_src.r, up_scale, deg)
        if res is not None:
            z = z + res.r
        return self.out('conv3x3_small', yd, z)

    def convt3x3s2(self, layer, x, act=RELU):
        yd = self.TG.convt3x3s2(self.tape, layer, x.d, act)
        z = F.conv_transpose2d(x.r, self.p(layer.weight), self.p(layer.bias), stride=2, padding=1, output_padding=1)
        return self.out('convt3x3s2', yd, z, act)

    def conv4x4s2(self, holder, x, **kw):
        yd = self.TG.conv4x4s2(self.tape, holder, x.d, **kw)
        return self.out('conv4x4s2', yd, F.conv2d(x.r, self.p(holder.weight), None, stride=2, padding=1))

    def backward_warp(self, x, flow, s2d=1, **kw):
        yd = self.TG.backward_warp(self.tape, x.d, flow.d, s2d=s2d, **kw)
        z = O.backward_warp(x.r, flow.r)
        return self.out('backward_warp', yd, z if s2d == 1 else O.space_to_depth(z, s2d))


# =================================================================================================
# conv3x3: the three data-gradient branches, activations, residual, two sources
# =================================================================================================
@pytest.mark.parametrize('act', [NONE, RELU, LRELU])
def test_conv3x3_data_gradient_small_kernel(ops, TG, monkeypatch, act):
    """3 -> 64: the data gradient onto an image is the small-cout kernel's shape."""
    t = Twin(TG)
    layer = conv(3, 64, 1)
    x = t.leaf(rs(2, (2, 3, 16, 24)))
    calls = counting(monkeypatch, ops, 'conv3x3_small', 'conv3x3_wino')
    y = t.conv3x3(layer, x, act)
    t.seed(y, 3)
    t.backward()
    assert len(calls['conv3x3_small']) == 1 and not calls['conv3x3_wino']
    assert (id(y.d) in t.tape.act_outputs) == (act != NONE)
    t.check('x', x)
    t.check_params()


@pytest.mark.parametrize('act,with_res', [(NONE, False), (RELU, False), (LRELU, False), (NONE, True)])
def test_conv3x3_data_gradient_mfma(ops, TG, monkeypatch, act, with_res):
    """64 -> 64 at 16 x 24: below the Winograd rule, the forward kernel on rot180-packed weights."""
    n, c, h, w = 2, 64, 16, 24
    assert not TG._prefers_wino(n, c, c, h, w)
    t = Twin(TG)
    layer = conv(c, c, 4)
    x = t.leaf(rs(5, (n, c, h, w)))
    res = t.leaf(rs(6, (n, c, h, w))) if with_res else None
    calls = counting(monkeypatch, ops, 'conv3x3', 'conv3x3_small', 'conv3x3_wino')
    y = t.conv3x3(layer, x, act, res=res)
    t.seed(y, 7)
    t.backward()
    assert len(calls['conv3x3']) == 2 and not calls['conv3x3_small'] and not calls['conv3x3_wino']
    t.check('x', x)
    if with_res:
        t.check('res', res)
    t.check_params()


def test_conv3x3_data_gradient_winograd(ops, TG, monkeypatch):
    """The smallest two-image 64 -> 64 shape (32 columns wide: one workgroup column) the rule sends to the Winograd
    form, forward and data gradient."""
    n, c, w = 2, 64, 32
    h = next(h for h in range(2, 2048, 2) if TG._prefers_wino(n, c, c, h, w))
    assert not TG._prefers_wino(n, c, c, h - 2, w)
    t = Twin(TG)
    layer = conv(c, c, 8)
    x = t.leaf(rs(9, (n, c, h, w)))
    calls = counting(monkeypatch, ops, 'conv3x3', 'conv3x3_wino')
    y = t.conv3x3(layer, x, LRELU)
    t.seed(y, 10)
    t.backward()
    assert len(calls['conv3x3_wino']) == 2 and not calls['conv3x3']
    t.check('x', x)
    t.check_params()


@pytest.mark.parametrize('need_dx,need_dx2', [(True, True), (False, True), (False, False)])
def test_conv3x3_two_sources(ops, TG, monkeypatch, need_dx, need_dx2):
    """cat[3, 48] -> 64 (SRNet's conv_in): one data gradient per source that asks for one; the bias gradient rides
    on ONE of the two deferred weight-gradient segments (it equals autograd's, not twice that)."""
    t = Twin(TG)
    layer = conv(51, 64, 11)
    x, x2 = t.leaf(rs(12, (2, 3, 16, 24)), need_dx), t.leaf(rs(13, (2, 48, 16, 24)), need_dx2)
    calls = counting(monkeypatch, ops, 'conv3x3', 'wgrad3x3')
    y = t.conv3x3(layer, x, RELU, x2=x2, need_dx=need_dx, need_dx2=need_dx2)
    t.seed(y, 14)
    t.backward()
    assert len(calls['conv3x3']) == 1 + int(need_dx) + int(need_dx2)
    with_bias = [k.get('bias_grad') is not None for _, k in calls['wgrad3x3']]
    assert len(with_bias) == 2 and sum(with_bias) == 1
    t.check('x', x) if need_dx else t.check_none(x)
    t.check('x2', x2) if need_dx2 else t.check_none(x2)
    t.check_params()


# =================================================================================================
# conv3x3_small: forward forms, both data-gradient kernels, the fused ReLU mask
# =================================================================================================
@pytest.mark.parametrize('form', ['res_small', 'res_mfma', 'up_bd4', 'up_bi2', 'tanh24', 'plain'])
def test_conv3x3_small_forward_forms(ops, TG, monkeypatch, form):
    n, cin, h, w = 2, 64, 12, 21 if form == 'res_mfma' else 20
    cout = 2 if form == 'tanh24' else 3
    t = Twin(TG)
    layer = conv(cin, cout, 15)
    x = t.leaf(rs(16, (n, cin, h, w)))
    calls = counting(monkeypatch, ops, 'conv3x3_small', 'conv3x3', 'conv3x3_fewin')
    if form.startswith('res'):
        res = t.leaf(rs(17, (n, cout, h, w)), grad=False)              # (data: no gradient)
        assert ops.conv3x3_small_res_ok(x.d, res.d) == (form == 'res_small')
        y = t.conv3x3_small(layer, x, NONE, res=res)
        assert (len(calls['conv3x3_small']), len(calls['conv3x3'])) == ((1, 0) if form == 'res_small' else (0, 1))
    elif form.startswith('up'):
        deg, s = ('BD', 4) if form == 'up_bd4' else ('BI', 2)
        up = t.leaf(rs(18, (n, cout, h // s, w // s), 0, 1), grad=False)
        y = t.conv3x3_small(layer, x, NONE, up_src=up, deg=deg, up_scale=s)
        assert len(calls['conv3x3_small']) == 1
    else:
        y = t.conv3x3_small(layer, x, TANH24 if form == 'tanh24' else NONE)
    t.seed(y, 19)
    n_fwd = len(calls['conv3x3'])
    t.backward()
    # 2 x 12 x 20 is below the size at which the few-channel kernel pays: the MFMA data gradient
    assert not ops.conv3x3_fewin_ok(y.d, cin) and not calls['conv3x3_fewin'] and len(calls['conv3x3']) == n_fwd + 1
    t.check('x', x)
    t.check_params()


def _fewin_shape(ops, fewin):
    """(n, cin, h, w) of the head's INPUT x0 (before the transposed conv doubles it) for each outcome of
    conv3x3_fewin_ok: the kernel wants 256 tiles of 4 x 64 pixels -- 64 images of 16 x 4 are the smallest such batch."""
    return (64, 16, 8, 2) if fewin else (2, 64, 8, 12)


@pytest.mark.parametrize('fewin', [False, True])
def test_conv3x3_small_data_gradient_kernels(ops, TG, monkeypatch, fewin):
    """Both outcomes of conv3x3_fewin_ok, no mask."""
    n, cin, h, w = _fewin_shape(ops, fewin)
    t = Twin(TG)
    layer = conv(cin, 3, 20)
    x = t.leaf(rs(21, (n, cin, 2 * h, 2 * w)))
    calls = counting(monkeypatch, ops, 'conv3x3_fewin', 'conv3x3')
    y = t.conv3x3_small(layer, x, NONE)
    assert ops.conv3x3_fewin_ok(y.d, cin) == fewin
    t.seed(y, 22)
    t.backward()
    assert (len(calls['conv3x3_fewin']), len(calls['conv3x3'])) == ((1, 0) if fewin else (0, 1))
    t.check('x', x)
    t.check_params()


@pytest.mark.parametrize('fewin', [False, True])
def test_conv3x3_small_fuses_the_relu_mask_of_a_transposed_conv(ops, TG, monkeypatch, fewin):
    """x = convt3x3s2(..., RELU): the head's data gradient applies the mask; it is the only contribution, so the
    transposed conv's node runs no act_bwd."""
    n, cin, h, w = _fewin_shape(ops, fewin)
    t = Twin(TG)
    up, head = conv(cin, cin, 23, transposed=True), conv(cin, 3, 24)
    x0 = t.leaf(rs(25, (n, cin, h, w)))
    calls = counting(monkeypatch, ops, 'act_bwd', 'conv3x3_fewin', 'conv3x3')
    x = t.convt3x3s2(up, x0, RELU)
    y = t.conv3x3_small(head, x, NONE)
    assert ops.conv3x3_fewin_ok(y.d, cin) == fewin
    t.seed(y, 26)
    t.backward()
    assert not calls['act_bwd'] and id(x.d) not in t.tape.unmasked
    masked = calls['conv3x3_fewin'] if fewin else calls['conv3x3']
    assert len(calls['conv3x3_fewin']) == int(fewin) and masked[-1][1].get('relu_mask') is x.d
    t.check('x0', x0)
    t.check_params()


@pytest.mark.parametrize('head_last', [True, False])
def test_masked_and_unmasked_contributions_to_one_relu_output(ops, TG, monkeypatch, head_last):
    """A second, unmasked consumer of the transposed conv's output, in both recording orders: the mask is then applied
    by the transposed conv's own act_bwd (ReLU' is idempotent on the part that came masked)."""
    t = Twin(TG)
    up, head, other = conv(64, 64, 27, transposed=True), conv(64, 3, 28), conv(64, 64, 29)
    x0 = t.leaf(rs(30, (2, 64, 8, 12)))
    calls = counting(monkeypatch, ops, 'act_bwd')
    x = t.convt3x3s2(up, x0, RELU)
    if head_last:
        z = t.conv3x3(other, x)
        y = t.conv3x3_small(head, x, NONE)
    else:
        y = t.conv3x3_small(head, x, NONE)
        z = t.conv3x3(other, x)
    t.seed(y, 31)
    t.seed(z, 32)
    t.backward()
    assert len(calls['act_bwd']) == 1 and id(x.d) in t.tape.unmasked
    t.check('x0', x0)
    t.check_params()


# =================================================================================================
# convt3x3s2
# =================================================================================================
@pytest.mark.parametrize('ci,co,act', [(64, 64, RELU), (24, 40, NONE), (128, 64, RELU), (128, 12, LRELU), (64, 128, RELU)])
def test_convt3x3s2_branches(ops, TG, monkeypatch, ci, co, act):
    """(64, 64), (24, 40): the data gradient as a stride-2 conv of dZ, dW straight from dZ.  ci or co = 128: past
    conv3x3s2_supported -- the space-to-depth embedding, phase-restricted (co % 8 == 0) or dense (co = 12); ci = 128:
    dW through the embedded gradient and the `post` hook, the bias gradient deferred on its own."""
    n, h, w = 2, 8, 12
    t = Twin(TG)
    layer = conv(ci, co, 33, transposed=True)
    x = t.leaf(rs(34, (n, ci, h, w)))
    calls = counting(monkeypatch, ops, 'conv3x3s2', 'conv3x3_phased', 'conv3x3', 'wgrad3x3_convt_multi',
                     'wgrad3x3_multi', 'wgrad3x3', 'index_gather', 'bias_grad')
    y = t.convt3x3s2(layer, x, act)
    t.seed(y, 35)
    gathers = len(calls['index_gather'])
    t.backward()
    direct_dx = ops.conv3x3s2_supported(n, co, ci, h, w)
    assert direct_dx == (ci <= 64 and co <= 64)                     # both outcomes are in the parameter list
    assert (len(calls['conv3x3s2']), len(calls['conv3x3_phased']), len(calls['conv3x3'])) == \
        ((1, 0, 0) if direct_dx else (0, 1, 0) if co % 8 == 0 else (0, 0, 1))
    if ci <= 64 and co <= 64:
        assert len(calls['wgrad3x3_convt_multi']) == 1 and not calls['wgrad3x3_multi'] and not calls['wgrad3x3']
    else:
        assert not calls['wgrad3x3_convt_multi'] and len(calls['wgrad3x3_multi']) + len(calls['wgrad3x3']) == 1
        assert len(calls['index_gather']) > gathers and len(calls['bias_grad']) == 1
    t.check('x', x)
    t.check_params()


def test_convt3x3s2_writes_into_a_reserved_buffer(ops, TG):
    t = Twin(TG)
    layer = conv(64, 64, 36, transposed=True)
    x = t.leaf(rs(37, (2, 64, 8, 12)))
    assert ops.conv3x3s2_supported(2, 64, 64, 8, 12)
    y = t.convt3x3s2(layer, x, RELU)
    block = torch.full((3, 2, 64, 8, 12), 7.0, device='cuda')
    t.tape.reserved[id(x.d)] = block[1]
    t.seed(y, 38)
    t.backward()
    assert t.tape.grad(x.d).data_ptr() == block[1].data_ptr()
    assert (block[0] == 7.0).all() and (block[2] == 7.0).all()
    t.check('x', x)
    t.check_params()


# =================================================================================================
# conv4x4s2
# =================================================================================================
@pytest.mark.parametrize('form,ci,co,w', [('direct', 64, 64, 32), ('sparse', 64, 64, 32), ('sparse', 64, 64, 24),
                                          ('dense', 12, 64, 24), ('dense', 64, 32, 24)])
def test_conv4x4s2_forms(ops, TG, monkeypatch, form, ci, co, w):
    n, h = 2, 16
    if form == 'sparse':
        monkeypatch.setenv('TG_CONV4_DIRECT', '0')
    assert (TG.direct_conv4() and ops.conv4x4s2_supported(n, ci, co, h, w)) == (form == 'direct')
    t = Twin(TG)
    layer = conv4(ci, co, 39)
    x = t.leaf(rs(40, (n, ci, h, w)))
    calls = counting(monkeypatch, ops, 'conv4x4s2', 'conv4x4s2_dgrad', 'conv3x3_phased', 'conv3x3')
    y = t.conv4x4s2(layer, x)
    t.seed(y, 41)
    t.backward()
    if form == 'direct':
        assert len(calls['conv4x4s2']) == 1 and len(calls['conv4x4s2_dgrad']) == 1
        assert not calls['conv3x3_phased'] and not calls['conv3x3']
    else:
        assert not calls['conv4x4s2'] and not calls['conv4x4s2_dgrad']
        fwd_phased = ci % 8 == 0 and co > 32
        assert len(calls['conv3x3_phased']) == int(fwd_phased) + int(ci % 64 == 0)
        assert len(calls['conv3x3']) == int(not fwd_phased) + int(ci % 64 != 0)
    t.check('x', x)
    t.check_params()


@pytest.mark.parametrize('act', [RELU, LRELU])
@pytest.mark.parametrize('w', [32, 24])
@pytest.mark.parametrize('order', ['strided_first', 'strided_second', 'two_strided'])
def test_conv4x4s2_on_an_activation_output(ops, TG, monkeypatch, act, w, order):
    """x = act(conv3x3(.)) read by a strided conv (w = 32: the direct kernels, 24: the embedding) and a second
    consumer.  strided_first: its gradient arrives first with act'(x) fused, the other contribution is brought to the
    same form.  strided_second: a gradient is already there, nothing is fused.  two_strided: the second strided conv
    finds a gradient, stays unfused and is brought to the form of the first -- with LeakyReLU a factor applied twice
    (0.04 instead of 0.2) would show."""
    n, h = 2, 16
    t = Twin(TG)
    c3, c4, other = conv(16, 64, 42), conv4(64, 64, 43), conv(64, 64, 44)
    c4b = conv4(64, 64, 45) if order == 'two_strided' else None
    x0 = t.leaf(rs(46, (n, 16, h, w)))
    calls = counting(monkeypatch, ops, 'act_bwd', 'conv4x4s2_dgrad', 'depth_to_space')
    x = t.conv3x3(c3, x0, act)
    if order == 'strided_first':                 # recorded last: its backward runs first
        outs = [t.conv3x3(other, x), t.conv4x4s2(c4, x)]
    elif order == 'strided_second':
        outs = [t.conv4x4s2(c4, x), t.conv3x3(other, x)]
    else:
        outs = [t.conv4x4s2(c4b, x), t.conv4x4s2(c4, x)]
    for i, o in enumerate(outs):
        t.seed(o, 47 + i)
    t.backward()
    direct = ops.conv4x4s2_supported(n, 64, 64, h, w)
    assert direct == (w == 32)
    fused = [k.get('act_y') is not None for _, k in calls['conv4x4s2_dgrad' if direct else 'depth_to_space']]
    if order == 'strided_first':
        assert fused == [True] and id(x.d) in t.tape.act_applied and len(calls['act_bwd']) == 1
    elif order == 'strided_second':
        assert fused == [False] and id(x.d) not in t.tape.act_applied and len(calls['act_bwd']) == 1
    else:
        assert fused == [True, False] and id(x.d) in t.tape.act_applied and len(calls['act_bwd']) == 1
    t.check('x0', x0)
    t.check_params()


# =================================================================================================
# point-wise nodes, linear1, BatchNorm + LeakyReLU
# =================================================================================================
def test_maxpool2_node(ops, TG):
    t = Twin(TG)
    x = t.leaf(TR.distinct_windows(50, (2, 5, 9, 13)))
    y = t.out('maxpool2', TG.maxpool2(t.tape, x.d), F.max_pool2d(x.r, 2, 2), tol=0.0)
    t.seed(y, 51)
    t.backward()
    assert torch.equal(t.tape.grad(x.d).cpu().double(), x.r.grad)          # a gradient is routed, never summed


@pytest.mark.parametrize('h,w', [(3, 5), (9, 13)])
@pytest.mark.parametrize('deg,s,mul', [('BD', 2, 2.0), ('BD', 4, 4.0), ('BI', 2, 1.0)])
def test_upsample_node(ops, TG, h, w, deg, s, mul):
    t = Twin(TG)
    x = t.leaf(rs(52, (2, 3, h, w)))
    y = t.out('upsample', TG.upsample(t.tape, x.d, s, ops.UP_MODE[deg], mul), mul * O.upsample(x.r, s, deg))
    t.seed(y, 53)
    t.backward()
    t.check('x', x, tol=1e-5)                                              # (test_upsample_bwd's number)


@pytest.mark.parametrize('s', [2, 4])
def test_space_to_depth_and_view_nodes(ops, TG, s):
    t = Twin(TG)
    x = t.leaf(rs(54, (2, 3, 8, 12)))
    y = t.out('space_to_depth', TG.space_to_depth(t.tape, x.d, s), O.space_to_depth(x.r, s), tol=0.0)
    shape = (2, 3 * s * s * (8 // s), 12 // s)
    v = t.out('view', TG.view(t.tape, y.d, shape), y.r.view(shape), tol=0.0)
    t.seed(v, 55)
    t.seed(y, 56)                                                          # a second contribution, on the un-viewed tensor
    t.backward()
    got, ref = t.tape.grad(x.d).cpu().double(), x.r.grad
    assert (got - ref).abs().max().item() <= 2.0 ** -24 * ref.abs().max().item()   # one fp32 addition


def test_channel_norm_node(ops, TG):
    t = Twin(TG)
    x = t.leaf(rs(57, (2, 3, 9, 13), 0, 1))
    mean, std = torch.tensor([0.485, 0.456, 0.406]), torch.tensor([0.229, 0.224, 0.225])
    y = t.out('channel_norm', TG.channel_norm(t.tape, x.d, mean.cuda(), std.cuda()),
              (x.r - mean.double().view(1, 3, 1, 1)) / std.double().view(1, 3, 1, 1))
    t.seed(y, 58)
    t.backward()
    t.check('x', x, tol=1e-6)                                              # one division per element


@pytest.mark.parametrize('need_dx,frozen', [(True, False), (False, False), (True, True)])
def test_linear1_node(ops, TG, need_dx, frozen):
    from tecogan_pytorch_amd.models.networks.tecogan_nets import _Linear1
    torch.manual_seed(59)
    lin = _Linear1(1001).cuda()
    if frozen:
        lin.requires_grad_(False)
    t = Twin(TG)
    x = t.leaf(rs(60, (5, 1001)), need_dx)
    y = t.out('linear1', TG.linear1(t.tape, lin, x.d, need_dx=need_dx),
              F.linear(x.r, t.p(lin.weight), t.p(lin.bias)), tol=2e-6)
    t.seed(y, 61)
    t.backward()
    t.check('x', x) if need_dx else t.check_none(x)
    t.check_params()


@pytest.mark.parametrize('groups,sync', [(1, False), (2, False), (1, True), (2, True)])
@pytest.mark.parametrize('need_dx,frozen', [(True, False), (False, False), (True, True)])
def test_bn_lrelu_node(ops, TG, groups, sync, need_dx, frozen):
    """groups = 2: two separate float64 batch-norm passes over the halves -- dgamma / dbeta are the sums over both,
    the running statistics are updated twice, in order (sync=True at world size 1 is the SyncBatchNorm path)."""
    from tecogan_pytorch_amd.models.networks.tecogan_nets import _BN
    n, c, h, w = 4, 8, 6, 5
    bn = _BN(c).cuda()
    with torch.no_grad():
        bn.weight.copy_(1 + 0.2 * rs(62, (c,))); bn.bias.copy_(0.1 * rs(63, (c,)))
        bn.running_mean.copy_(0.3 * rs(64, (c,))); bn.running_var.copy_(1 + 0.5 * rs(65, (c,)))
    if frozen:
        bn.weight.requires_grad_(False); bn.bias.requires_grad_(False)
    rm, rv = bn.running_mean.cpu().double(), bn.running_var.cpu().double()
    xs = rs(66, (n, c, h, w), -2, 2)
    xs[n // 2:] = xs[n // 2:] * 1.5 + 0.7                                  # the two groups have their own statistics
    t = Twin(TG)
    x = t.leaf(xs, need_dx)
    yd = TG.bn_lrelu(t.tape, bn, x.d, need_dx=need_dx, sync=sync, groups=groups)
    per = n // groups
    z = torch.cat([F.batch_norm(x.r[g * per:(g + 1) * per], rm, rv, t.p(bn.weight), t.p(bn.bias), True, 0.1, 1e-5)
                   for g in range(groups)])
    y = t.out('bn_lrelu', yd, z, LRELU)
    assert relerr(bn.running_mean, rm) <= 1e-5 and relerr(bn.running_var, rv) <= 1e-5
    assert bn._pending == groups
    t.seed(y, 67)
    t.backward()
    t.check('x', x) if need_dx else t.check_none(x)
    t.check_params()


# =================================================================================================
# backward_warp node
# =================================================================================================
def _warp_leaves(t, shape, s2d=1, flow_grad=True):
    x, flow, _, _, _ = TR.warp_inputs(70, shape, TR.OUT_FRAC, s2d)
    return t.leaf(x), t.leaf(flow, flow_grad)


@pytest.mark.parametrize('s2d', [1, 2, 4])
def test_backward_warp_node_fresh_gradient(ops, TG, s2d):
    t = Twin(TG)
    x, flow = _warp_leaves(t, (2, 3, 16, 40), s2d)
    y = t.backward_warp(x, flow, s2d=s2d)
    t.seed(y, 71)
    t.backward()
    t.check('x', x)
    t.check('flow', flow)


@pytest.mark.parametrize('s2d', [1, 2])
def test_backward_warp_node_adds_into_the_gradient_x_holds(ops, TG, monkeypatch, s2d):
    t = Twin(TG)
    x, flow = _warp_leaves(t, (2, 3, 16, 40), s2d)
    calls = counting(monkeypatch, ops, 'backward_warp_bwd', 'axpy_')
    y = t.backward_warp(x, flow, s2d=s2d)
    t.seed(y, 72)
    t.seed(x, 73)                                                          # x's own loss term
    held = t.tape.grad(x.d)
    t.backward()
    assert t.tape.grad(x.d) is held and not calls['axpy_']
    assert calls['backward_warp_bwd'][0][1].get('dimg_acc') is held
    t.check('x', x)
    t.check('flow', flow)


def test_backward_warp_node_falls_back_on_a_strided_gradient(ops, TG, monkeypatch):
    """x holds a NON-contiguous gradient: no scatter into it; a fresh image gradient is accumulated instead."""
    t = Twin(TG)
    x, flow = _warp_leaves(t, (2, 3, 16, 40))
    calls = counting(monkeypatch, ops, 'backward_warp_bwd')
    y = t.backward_warp(x, flow)
    t.seed(y, 74)
    g0 = rs(75, (2, 3, 16, 80))
    t.tape.add_grad(x.d, g0.cuda()[:, :, :, ::2])
    t.loss = t.loss + (x.r * g0[:, :, :, ::2].double()).sum()
    assert not t.tape.grad(x.d).is_contiguous()
    t.backward()
    assert calls['backward_warp_bwd'][0][1].get('dimg_acc') is None
    t.check('x', x)
    t.check('flow', flow)


def test_backward_warp_node_falls_back_on_an_act_applied_tensor(ops, TG, monkeypatch):
    """x = lrelu(conv3x3(.)) whose gradient arrived with act'(x) applied (a direct strided conv, recorded last): the
    scatter of raw image gradients must not add into it -- the fallback brings them to the same form first."""
    n, h, w = 2, 16, 32
    t = Twin(TG)
    c3, c4 = conv(16, 64, 76), conv4(64, 64, 77)
    x0 = t.leaf(rs(78, (n, 16, h, w)))
    flow = t.leaf(TR.kinkfree_flow(79, n, h, w, TR.OUT_FRAC)[0])
    calls = counting(monkeypatch, ops, 'backward_warp_bwd', 'act_bwd')
    x = t.conv3x3(c3, x0, LRELU)
    y = t.backward_warp(x, flow)
    z = t.conv4x4s2(c4, x)
    t.seed(y, 80)
    t.seed(z, 81)
    t.backward()
    assert id(x.d) in t.tape.act_applied and calls['backward_warp_bwd'][0][1].get('dimg_acc') is None
    assert len(calls['act_bwd']) == 1
    t.check('x0', x0)
    t.check('flow', flow)
    t.check_params()


@pytest.mark.parametrize('s2d', [1, 4])
def test_backward_warp_node_flow_gradient_into_a_callers_buffer(ops, TG, s2d):
    t = Twin(TG)
    x, flow = _warp_leaves(t, (2, 3, 16, 40), s2d)
    big = torch.full((3, 2, 2, 16, 40), 7.0, device='cuda')
    y = t.backward_warp(x, flow, s2d=s2d, dflow_out=lambda: big[1])
    t.seed(y, 82)
    t.backward()
    assert t.tape.grad(flow.d) is None                                     # nothing lands on the tape for `flow`
    assert relerr(big[1], flow.r.grad) <= TOL and (big[0] == 7.0).all() and (big[2] == 7.0).all()
    t.check('x', x)


def test_backward_warp_node_without_an_image_gradient(ops, TG, monkeypatch):
    t = Twin(TG)
    x, flow = _warp_leaves(t, (2, 3, 16, 40))
    x = V(x.d, x.r.detach())
    calls = counting(monkeypatch, ops, 'backward_warp_bwd')
    y = t.backward_warp(x, flow, need_dimg=False)
    t.seed(y, 83)
    t.backward()
    assert t.tape.grad(x.d) is None and calls['backward_warp_bwd'][0][0][3] is False
    t.check('flow', flow)


# =================================================================================================
# the deferred weight-gradient flush
# =================================================================================================
def test_flush_one_launch_over_equal_shapes(ops, TG, monkeypatch):
    t = Twin(TG)
    layer = conv(64, 64, 84)
    xs = [t.leaf(rs(85 + i, (2, 64, 12, 20))) for i in range(3)]
    calls = counting(monkeypatch, ops, 'wgrad3x3_multi', 'wgrad3x3')
    for i, x in enumerate(xs):
        t.seed(t.conv3x3(layer, x, RELU), 88 + i)
    t.backward()
    assert not calls['wgrad3x3'] and [len(a[0]) for a, _ in calls['wgrad3x3_multi']] == [3]
    for i, x in enumerate(xs):
        t.check(f'x{i}', x)
    t.check_params()


def test_flush_concatenates_unequal_batches(ops, TG, monkeypatch):
    t = Twin(TG)
    layer = conv(64, 64, 91)
    xs = [t.leaf(rs(92, (2, 64, 12, 20))), t.leaf(rs(93, (3, 64, 12, 20)))]
    calls = counting(monkeypatch, ops, 'wgrad3x3')
    for i, x in enumerate(xs):
        t.seed(t.conv3x3(layer, x, LRELU), 94 + i)
    t.backward()
    assert [a[0].shape[0] for a, _ in calls['wgrad3x3']] == [5]
    for i, x in enumerate(xs):
        t.check(f'x{i}', x)
    t.check_params()


def test_flush_transposed_conv_pair_by_pair_on_unequal_shapes(ops, TG, monkeypatch):
    t = Twin(TG)
    layer = conv(64, 64, 96, transposed=True)
    xs = [t.leaf(rs(97, (2, 64, 8, 12))), t.leaf(rs(98, (2, 64, 6, 10)))]
    calls = counting(monkeypatch, ops, 'wgrad3x3_convt_multi')
    for i, x in enumerate(xs):
        t.seed(t.convt3x3s2(layer, x, RELU), 99 + i)
    t.backward()
    assert [len(a[0]) for a, _ in calls['wgrad3x3_convt_multi']] == [1, 1]
    for i, x in enumerate(xs):
        t.check(f'x{i}', x)
    t.check_params()


def test_flush_with_frozen_layers(ops, TG, monkeypatch):
    """No gradient buffer is created for a frozen layer of any kind, nothing is deferred, the data gradients are right."""
    t = Twin(TG)
    c3, ct, c4 = conv(16, 64, 101, frozen=True), conv(64, 64, 102, transposed=True, frozen=True), \
        conv4(64, 64, 103, frozen=True)
    head = conv(64, 3, 104, frozen=True)
    x0 = t.leaf(rs(105, (2, 16, 8, 16)))
    calls = counting(monkeypatch, ops, 'wgrad3x3_multi', 'wgrad3x3', 'wgrad3x3_convt_multi', 'bias_grad')
    a = t.conv3x3(c3, x0, LRELU)
    b = t.convt3x3s2(ct, a, RELU)
    t.seed(t.conv4x4s2(c4, b), 106)
    t.seed(t.conv3x3_small(head, b, TANH24), 107, mul=0.05)
    assert not t.tape.deferred
    t.backward()
    assert not any(calls.values())
    t.check('x0', x0)
    t.check_params()
