"""The flush of the tape's deferred parameter gradients (models/train_graph.py) against a recording fake of `ops`:
which library wrapper every kind of deferred work ends in, with which operands, and in which order.  No GPU and no
library: the entries are CPU tensors of a few channels at 4 x 6 pixels and nothing is computed.

A trace line is (function, p operand, q operand, gradient buffer, cb_off, accumulate, phased, bias buffer): an operand is
the list of its segments' shapes (the multi-segment kernels) or one shape (one tensor, concatenated where the segments
could not stay where they lie); a buffer is the name the test gave it, or ('temp', shape) for one the flush allocated."""
import pytest
import torch

import tecogan_pytorch_amd  # noqa: F401
from tecogan_pytorch_amd.models import train_graph as TG

H, W = 4, 6


def t(n, c, h=H, w=W):
    return torch.zeros(n, c, h, w)


def strided(n, c):
    """The shape of t(n, c), not contiguous."""
    x = torch.zeros(n, c, H, 2 * W)[..., ::2]
    assert x.shape == (n, c, H, W) and not x.is_contiguous()
    return x


class FakeOps:
    def __init__(self):
        self.trace, self.names, self.temps = [], {}, []

    def named(self, name, tensor):
        self.names[id(tensor)] = name
        return tensor

    def _buf(self, b):
        if b is None:
            return None
        if id(b) not in self.names:
            self.temps.append(b)
            return ('temp', tuple(b.shape))
        return self.names[id(b)]

    @staticmethod
    def _operand(v):
        if isinstance(v, list):
            assert all(x.is_contiguous() for x in v)
            return [tuple(x.shape) for x in v]
        assert v.is_contiguous()
        return tuple(v.shape)

    def _wgrad(self, fn, p, q, grad, cb_off, accumulate, phased, bias_grad):
        self.trace.append((fn, self._operand(p), self._operand(q), self._buf(grad), cb_off, accumulate, phased,
                           self._buf(bias_grad)))
        return grad

    def wgrad3x3(self, p, q, grad, cb_off=0, accumulate=True, bias_grad=None):
        assert torch.is_tensor(p) and torch.is_tensor(q)
        return self._wgrad('wgrad3x3', p, q, grad, cb_off, accumulate, None, bias_grad)

    def wgrad3x3_multi(self, p_list, q_list, grad, cb_off=0, accumulate=True, phased=None, bias_grad=None):
        assert isinstance(p_list, list) and isinstance(q_list, list)
        return self._wgrad('wgrad3x3_multi', p_list, q_list, grad, cb_off, accumulate, phased, bias_grad)

    def wgrad3x3_convt_multi(self, x_list, dz_list, grad, accumulate=True, bias_grad=None):
        assert isinstance(x_list, list) and isinstance(dz_list, list)
        return self._wgrad('wgrad3x3_convt_multi', x_list, dz_list, grad, None, accumulate, None, bias_grad)

    def wgrad3x3_body(self, dz_list, acts_list, grads, accumulate=True, dbs=None):
        self.trace.append(('wgrad3x3_body', self._operand(dz_list), self._operand(acts_list),
                           [self._buf(g) for g in grads], None, accumulate, None, [self._buf(b) for b in dbs]))
        return grads

    def bias_grad_multi(self, dy_list, db, accumulate=True):
        assert isinstance(dy_list, list)
        self.trace.append(('bias_grad_multi', self._operand(dy_list), None, self._buf(db), None, accumulate, None, None))
        return db

    def bias_grad(self, dy, db, accumulate=True):
        assert torch.is_tensor(dy)
        self.trace.append(('bias_grad', self._operand(dy), None, self._buf(db), None, accumulate, None, None))
        return db


@pytest.fixture
def fake(monkeypatch):
    f = FakeOps()
    monkeypatch.setattr(TG, 'ops', f)
    return f


def flushed(tape):
    tape.flush_deferred()
    assert not tape.deferred and not tape.deferred_body and not tape.deferred_bias
    return TG.ops.trace


S = (2, 5, H, W)        # the (dZ, x) shapes of the plain cases: 5 channels out, 3 in
X = (2, 3, H, W)


# ---- plain --------------------------------------------------------------------------------------------------------
def test_plain_uniform_pairs_take_one_multi_segment_launch(fake):
    tape, gw, gb = TG.Tape(), fake.named('gw', torch.zeros(5, 3, 3, 3)), fake.named('gb', torch.zeros(5))
    for _ in range(3):
        tape.defer_wgrad('k', t(2, 5), t(2, 3), gw, 0, bias=gb)
    assert flushed(tape) == [('wgrad3x3_multi', [S] * 3, [X] * 3, 'gw', 0, True, None, 'gb')]


def test_plain_single_pairs_of_a_two_source_layer(fake):
    """One pair: the tensor itself.  The second source lands at its channel offset, the bias rides on one of the two."""
    tape, gw, gb = TG.Tape(), fake.named('gw', torch.zeros(5, 7, 3, 3)), fake.named('gb', torch.zeros(5))
    dz = t(2, 5)
    tape.defer_wgrad(('w', 1, 0), dz, t(2, 3), gw, 0, bias=None)
    tape.defer_wgrad(('w', 1, 1), dz, t(2, 4), gw, 3, bias=gb)
    assert flushed(tape) == [('wgrad3x3', S, X, 'gw', 0, True, None, None),
                             ('wgrad3x3', S, (2, 4, H, W), 'gw', 3, True, None, 'gb')]


@pytest.mark.parametrize('second', ['larger_batch', 'strided'])
def test_plain_pairs_that_are_not_uniform_are_concatenated(fake, second):
    tape, gw = TG.Tape(), fake.named('gw', torch.zeros(5, 3, 3, 3))
    tape.defer_wgrad('k', t(2, 5), t(2, 3), gw, 2)
    if second == 'larger_batch':
        tape.defer_wgrad('k', t(3, 5), t(3, 3), gw, 2)
    else:
        tape.defer_wgrad('k', t(3, 5)[:2], strided(2, 3), gw, 2)
    n = 5 if second == 'larger_batch' else 4
    assert flushed(tape) == [('wgrad3x3', (n, 5, H, W), (n, 3, H, W), 'gw', 2, True, None, None)]


# ---- embedded -----------------------------------------------------------------------------------------------------
def embedded(tape, key, pairs, phased, seen):
    for p, q in pairs:
        tape.defer_wgrad_embedded(key, p, q, seen.append, phased=phased)


@pytest.mark.parametrize('pairs, phased, expect', [
    # the kernel dispatches on 64-channel blocks: phased kept, a single pair counts as uniform
    (2, (64, 5, 6), ('wgrad3x3_multi', [S] * 2, [(2, 12, H, W)] * 2, ('temp', (5, 12, 3, 3)), 0, False, (64, 5, 6), None)),
    (1, (64, 5, 6), ('wgrad3x3_multi', [S], [(2, 12, H, W)], ('temp', (5, 12, 3, 3)), 0, False, (64, 5, 6), None)),
    # phased dropped
    (2, (8, 5, 6), ('wgrad3x3_multi', [S] * 2, [(2, 12, H, W)] * 2, ('temp', (5, 12, 3, 3)), 0, False, None, None)),
    (1, (8, 5, 6), ('wgrad3x3', S, (2, 12, H, W), ('temp', (5, 12, 3, 3)), 0, False, None, None)),
    (2, None, ('wgrad3x3_multi', [S] * 2, [(2, 12, H, W)] * 2, ('temp', (5, 12, 3, 3)), 0, False, None, None)),
    (1, None, ('wgrad3x3', S, (2, 12, H, W), ('temp', (5, 12, 3, 3)), 0, False, None, None)),
])
def test_embedded_uniform_pairs(fake, pairs, phased, expect):
    tape, seen = TG.Tape(), []
    embedded(tape, ('c4', 1), [(t(2, 5), t(2, 12)) for _ in range(pairs)], phased, seen)
    assert flushed(tape) == [expect]
    # the scatter hook gets the temporary the launch wrote: (p channels, q channels, 3, 3)
    assert len(seen) == 1 and seen[0] is fake.temps[0] and seen[0].shape == (5, 12, 3, 3)
    assert seen[0].dtype == torch.float32


@pytest.mark.parametrize('phased', [(64, 5, 6), None])
def test_embedded_pairs_that_are_not_uniform_are_concatenated(fake, phased):
    tape, seen = TG.Tape(), []
    embedded(tape, ('ct', 1), [(t(2, 5), t(2, 12)), (t(2, 5), strided(2, 12))], phased, seen)
    assert flushed(tape) == [('wgrad3x3', (4, 5, H, W), (4, 12, H, W), ('temp', (5, 12, 3, 3)), 0, False, None, None)]
    assert seen[0] is fake.temps[0]


# ---- transposed-direct --------------------------------------------------------------------------------------------
def test_convt_uniform_pairs_take_one_launch(fake):
    tape, gw, gb = TG.Tape(), fake.named('gw', torch.zeros(3, 5, 3, 3)), fake.named('gb', torch.zeros(5))
    for _ in range(2):
        tape.defer_wgrad_convt(('ctw', 1), t(2, 3), t(2, 5, 2 * H, 2 * W), gw, gb)
    assert flushed(tape) == [('wgrad3x3_convt_multi', [X] * 2, [(2, 5, 2 * H, 2 * W)] * 2, 'gw', None, True, None, 'gb')]


@pytest.mark.parametrize('second', ['smaller_frame', 'strided'])
def test_convt_pairs_that_are_not_uniform_go_pair_by_pair(fake, second):
    tape, gw, gb = TG.Tape(), fake.named('gw', torch.zeros(3, 5, 3, 3)), fake.named('gb', torch.zeros(5))
    tape.defer_wgrad_convt(('ctw', 1), t(2, 3), t(2, 5, 2 * H, 2 * W), gw, gb)
    if second == 'smaller_frame':
        tape.defer_wgrad_convt(('ctw', 1), t(2, 3, 2, 3), t(2, 5, 4, 6), gw, gb)
        x2, d2 = (2, 3, 2, 3), (2, 5, 4, 6)
    else:
        tape.defer_wgrad_convt(('ctw', 1), strided(2, 3), t(2, 5, 2 * H, 2 * W), gw, gb)
        x2, d2 = X, (2, 5, 2 * H, 2 * W)
    assert flushed(tape) == [('wgrad3x3_convt_multi', [X], [(2, 5, 2 * H, 2 * W)], 'gw', None, True, None, 'gb'),
                             ('wgrad3x3_convt_multi', [x2], [d2], 'gw', None, True, None, 'gb')]


# ---- body and bias ------------------------------------------------------------------------------------------------
def body_layers(fake, tag, frozen=False):
    layers = [torch.nn.Conv2d(4, 4, 3, padding=1) for _ in range(3)]        # conv_in + one residual block
    for i, m in enumerate(layers):
        m.requires_grad_(not frozen)
        if not frozen:
            m.weight.grad = fake.named(f'{tag}w{i}', torch.zeros_like(m.weight))
            m.bias.grad = fake.named(f'{tag}b{i}', torch.zeros_like(m.bias))
    return layers


def test_body_one_launch_over_the_layers_behind_conv_in(fake):
    tape, layers = TG.Tape(), body_layers(fake, 'g')
    for _ in range(2):
        tape.defer_body(7, layers, torch.zeros(3, 2, 4, H, W), torch.zeros(3, 2, 4, H, W))
    assert flushed(tape) == [('wgrad3x3_body', [(3, 2, 4, H, W)] * 2, [(3, 2, 4, H, W)] * 2, ['gw1', 'gw2'], None, True,
                              None, ['gb1', 'gb2'])]


def test_frozen_body_is_skipped(fake):
    tape, layers = TG.Tape(), body_layers(fake, 'g', frozen=True)
    tape.defer_body(7, layers, torch.zeros(3, 2, 4, H, W), torch.zeros(3, 2, 4, H, W))
    assert flushed(tape) == []
    assert all(m.weight.grad is None and m.bias.grad is None for m in layers)


def test_two_bias_buffers_one_uniform_one_not(fake):
    tape, b1, b2, b3 = TG.Tape(), fake.named('b1', torch.zeros(5)), fake.named('b2', torch.zeros(5)), \
        fake.named('b3', torch.zeros(5))
    tape.defer_bias(b1, t(2, 5))
    tape.defer_bias(b2, t(2, 5))
    tape.defer_bias(b1, t(2, 5))
    tape.defer_bias(b2, strided(2, 5))
    tape.defer_bias(b3, t(2, 5))
    assert flushed(tape) == [('bias_grad_multi', [S] * 2, None, 'b1', None, True, None, None),
                             ('bias_grad', (4, 5, H, W), None, 'b2', None, True, None, None),
                             ('bias_grad', S, None, 'b3', None, True, None, None)]


# ---- order --------------------------------------------------------------------------------------------------------
def test_order_weights_by_first_deferral_then_bodies_then_biases(fake):
    tape, seen, layers = TG.Tape(), [], body_layers(fake, 'body_')
    ga, gb_, gc, bias = (fake.named(n, torch.zeros(s)) for n, s in
                         (('ga', (5, 3, 3, 3)), ('gb', (5, 3, 3, 3)), ('gc', (3, 5, 3, 3)), ('bias', (5,))))
    tape.defer_bias(bias, t(2, 5))
    tape.defer_body(7, layers, torch.zeros(3, 2, 4, H, W), torch.zeros(3, 2, 4, H, W))
    embedded(tape, ('ct', 1), [(t(2, 5), t(2, 12))], None, seen)
    tape.defer_wgrad(('w', 1, 0), t(2, 5), t(2, 3), ga, 0)
    tape.defer_wgrad_convt(('ctw', 2), t(2, 3), t(2, 5, 2 * H, 2 * W), gc, bias)
    tape.defer_wgrad(('w', 3, 0), t(2, 5), t(2, 3), gb_, 0)
    tape.defer_wgrad(('w', 1, 0), t(2, 5), t(2, 3), ga, 0)         # a later deferral does not move the key
    embedded(tape, ('ct', 1), [(t(2, 5), t(2, 12))], None, seen)
    assert [(line[0], line[3]) for line in flushed(tape)] == [
        ('wgrad3x3_multi', ('temp', (5, 12, 3, 3))), ('wgrad3x3_multi', 'ga'), ('wgrad3x3_convt_multi', 'gc'),
        ('wgrad3x3', 'gb'), ('wgrad3x3_body', ['body_w1', 'body_w2']), ('bias_grad', 'bias')]
    assert len(seen) == 1


def test_backward_flushes(fake):
    tape, gw, ran = TG.Tape(), fake.named('gw', torch.zeros(5, 3, 3, 3)), []
    tape.record(lambda: (ran.append(1), tape.defer_wgrad('k', t(2, 5), t(2, 3), gw, 0)))
    tape.backward()
    assert ran == [1] and not tape.nodes and not tape.deferred
    assert fake.trace == [('wgrad3x3', S, X, 'gw', 0, True, None, None)]
