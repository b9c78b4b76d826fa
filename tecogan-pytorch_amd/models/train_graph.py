"""A minimal reverse-mode tape whose every arithmetic node is a HIP kernel.

The reference trains through torch.autograd over ATen ops; here the training
graph of this one model family is recorded explicitly: each differentiable op
below runs its forward kernel, and registers a closure that runs the matching
backward kernels (conv data gradients reuse the forward MFMA kernel on
rot180-packed weights, weight gradients use the MFMA wgrad kernel, transposed
and strided convs go through their space-to-depth embedding).  torch is used
for storage and for pure data movement (slicing / stacking / zero fill) only.

Gradients of intermediate tensors are keyed by tensor identity; parameter
gradients accumulate into `param.grad` (allocated and zeroed by the caller).
"""
import os

import torch

from .. import ops
from . import packs
# (what moved next to the packed-weight store stays reachable here: tests and labs use these names)
from .packs import _K4, _KT, _conv4_embed, _convt_embed, _embed_index, prefers_wino as _prefers_wino  # noqa: F401
# (the fail-safe of the chained launches lives in train_chain; its names stay reachable here)
from .train_chain import (_ChainState, _distributed_world, chain_check, chain_epoch,  # noqa: F401
                          guard_available, stamp_fault)

NONE, RELU, LRELU, TANH24 = ops.ACT_NONE, ops.ACT_RELU, ops.ACT_LRELU02, ops.ACT_TANH24


class Tape:
    def __init__(self):
        self.nodes = []
        self.grads = {}
        self.keep = []          # tensors that must outlive backward (id() stability)
        self.deferred = {}
        self.deferred_bias = {}
        self.deferred_body = {}  # chained SRNet bodies: per network, the (acts, dz, g_out) blocks of every swept frame
        # ReLU-backward fused into the producer of a gradient: a ReLU layer registers its output in
        # `relu_outputs`; a node that delivers the gradient w.r.t. such a tensor may apply the mask in
        # its own epilogue and say so (add_grad(..., masked=True)); the ReLU layer then skips its
        # act_bwd pass unless some other contribution arrived unmasked.
        self.relu_outputs = set()
        self.unmasked = set()
        # the same idea for the generic conv node's activations (ReLU or LeakyReLU): a conv3x3 node
        # registers its activation output here; a producer of its gradient that can apply act'(.) itself
        # (the depth-to-space of a strided conv's data gradient) delivers it with act_applied=True and the
        # node skips act_bwd.  LeakyReLU' is not idempotent: add_grad brings any other contribution to the
        # same tensor to the same form before it accumulates.
        self.act_outputs = {}
        self.act_applied = set()
        # a consumer that will copy the gradient of t into a buffer of its own anyway (the chained body puts
        # the gradient of its output into the last slot of its dZ block) may reserve that buffer here; a
        # producer that can write into a given tensor then delivers the gradient in place
        self.reserved = {}

    # -- gradient bookkeeping -------------------------------------------------
    def add_grad(self, t, g, masked=False, act_applied=False):
        """Accumulate g into the gradient of t.  Takes ownership of g.  masked: g already carries
        the ReLU-backward mask of t (t is in relu_outputs).  act_applied: g already is the gradient of
        the pre-activation of t (t is in act_outputs)."""
        k = id(t)
        if not masked:
            self.unmasked.add(k)
        cur = self.grads.get(k)
        if act_applied or k in self.act_applied:
            # LeakyReLU' is not idempotent: every contribution must carry it exactly once
            a = self.act_outputs[k]
            if k in self.act_applied and not act_applied:
                g = ops.act_bwd(g, t, a, out=g)
            elif k not in self.act_applied and cur is not None:
                ops.act_bwd(cur, t, a, out=cur)
            self.act_applied.add(k)
        if cur is None:
            self.grads[k] = g
            self.keep.append(t)
        else:
            if not cur.is_contiguous():      # (a caller's strided first contribution: axpy_ walks flat memory)
                cur = self.grads[k] = cur.contiguous()
            ops.axpy_(cur, g if g.is_contiguous() else g.contiguous(), 1.0)

    def grad(self, t):
        return self.grads.get(id(t))

    def pop_grad(self, t):
        return self.grads.pop(id(t), None)

    def record(self, fn):
        self.nodes.append(fn)

    def backward(self):
        for fn in reversed(self.nodes):
            fn()
        self.nodes = []
        self.flush_deferred()

    # -- deferred parameter gradients -------------------------------------------
    # A layer is applied once per unrolled frame (19x for SRNet), each time on a small
    # image.  Its weight gradient is a sum over all applications, so the (dZ, X) pairs
    # are collected during the reverse sweep and reduced by ONE wgrad launch per layer
    # over the concatenated batch: 19x fewer launches / split-K reductions, and enough
    # pixel tiles per launch to fill the GPU.
    # One queue entry per key: (flush function of its kind, what the key's first deferral fixed, a list, b list); each
    # kind's function below names what its fields mean.  Weight gradients are flushed in order of first deferral.
    def _defer(self, queue, key, flush, fixed, a, b=None):
        ent = queue.get(key)
        if ent is None:
            ent = queue[key] = (flush, fixed, [], [])
        ent[2].append(a)
        ent[3].append(b)

    def defer_wgrad(self, key, dz, x, gw, cb_off=0, bias=None):
        """dW[:, cb_off:cb_off + channels of x] += dZ (*) x.  bias: the layer's bias-gradient buffer -- db = sum of dZ
        comes out of the same launch (instead of defer_bias: a second pass over every dZ)."""
        self._defer(self.deferred, key, _flush_plain, (gw, cb_off, bias), dz, x)

    def defer_wgrad_embedded(self, key, p, q, scatter, phased=None):
        """The (p channels, q channels, 3, 3) gradient of a space-to-depth embedding, made in a temporary that `scatter`
        adds into the layer's own gradient.  phased: (channels per phase, tap rows, tap columns) of the masked kernel."""
        self._defer(self.deferred, key, _flush_embedded, (scatter, phased), p, q)

    def defer_wgrad_convt(self, key, x, dz, gw, gb):
        """dW and db of a transposed conv straight from its input and dZ (at twice the resolution)."""
        self._defer(self.deferred, key, _flush_convt, (gw, gb), x, dz)

    def defer_bias(self, buf, dz):
        self._defer(self.deferred_bias, id(buf), _flush_bias, (buf,), dz)

    def defer_body(self, key, layers, acts, dz):
        self._defer(self.deferred_body, key, _flush_body, (layers,), dz, acts)

    def flush_deferred(self):
        for queue in (self.deferred, self.deferred_body, self.deferred_bias):
            for flush, fixed, a, b in queue.values():
                flush(a, b, *fixed)
            queue.clear()


def _uniform(*lists):
    """Every list's tensors share one shape and are contiguous: a multi-segment kernel reads them where they lie."""
    return all(t.shape == ts[0].shape and t.is_contiguous() for ts in lists for t in ts)


def _joined(ts):
    return ts[0] if len(ts) == 1 else torch.cat(ts, 0)


def _wgrad(ps, qs, grad, phased=None, **kw):
    """One weight-gradient launch over the pairs: the per-frame tensors where they lie, else their concatenation."""
    uniform = _uniform(ps, qs)
    if phased is not None and phased[0] % 64 == 0 and uniform:     # (the kernel dispatches on 64-channel blocks)
        ops.wgrad3x3_multi(ps, qs, grad, phased=phased, **kw)      # skips the taps a sub-pixel phase does not own
    elif len(ps) > 1 and uniform:
        ops.wgrad3x3_multi(ps, qs, grad, **kw)
    else:
        ops.wgrad3x3(_joined(ps), _joined(qs), grad, **kw)


def _flush_plain(dzs, xs, gw, cb_off, bias):
    _wgrad(dzs, xs, gw, cb_off=cb_off, accumulate=True, bias_grad=bias)


def _flush_embedded(ps, qs, scatter, phased):
    # accumulate=False: every tap the scatter hook reads is overwritten
    ge = torch.empty(ps[0].shape[1], qs[0].shape[1], 3, 3, dtype=torch.float32, device=ps[0].device)
    _wgrad(ps, qs, ge, phased=phased, accumulate=False)
    scatter(ge)


def _flush_convt(xs, dzs, gw, gb):
    if _uniform(xs, dzs):
        ops.wgrad3x3_convt_multi(xs, dzs, gw, accumulate=True, bias_grad=gb)
    else:
        for x, dz in zip(xs, dzs):
            ops.wgrad3x3_convt_multi([x.contiguous()], [dz.contiguous()], gw, accumulate=True, bias_grad=gb)


def _flush_body(dz_blocks, act_blocks, layers):
    """The 2*nb residual-block convs of every swept frame of a chained body: ONE weight-gradient launch (+ one reduce)
    and one bias-gradient launch instead of 2*nb of each per flush."""
    if layers[1].weight.requires_grad:
        ops.wgrad3x3_body(dz_blocks, act_blocks, [_grad_buf(m.weight) for m in layers[1:]],
                          dbs=[_grad_buf(m.bias) for m in layers[1:]])


def _flush_bias(dzs, _, buf):
    if len(dzs) > 1 and _uniform(dzs):
        ops.bias_grad_multi(dzs, buf, accumulate=True)
    else:
        ops.bias_grad(_joined(dzs), buf, accumulate=True)


def _grad_buf(p):
    if p.grad is None:
        p.grad = torch.zeros_like(p)
    return p.grad


# ---------------------------------------------------------------------------
# conv3x3 (+bias, +activation, two-source input, residual)
# ---------------------------------------------------------------------------
def conv3x3(tape, layer, x, act=NONE, x2=None, res=None, need_dx=True, need_dx2=True):
    w, b = layer.weight, layer.bias
    cout, cin = w.shape[0], w.shape[1]
    n_, c1, h_, w_ = x.shape
    y = packs.conv3x3_forward(layer, x, act, x2, res)    # (D's conv_in, VGG19 on the HR frames: Winograd form)
    if tape is None:
        return y
    if act in (RELU, LRELU) and res is None:
        tape.act_outputs[id(y)] = act

    def bwd():
        g = tape.pop_grad(y)
        if g is None:
            return
        if res is not None:
            tape.add_grad(res, g.clone())
        if id(y) in tape.act_applied:            # the producer of g applied act'(.) already
            dz = g
        else:
            dz = ops.act_bwd(g, y, act, out=g) if act != NONE else g
        if w.requires_grad:
            gw = _grad_buf(w)
            # (the bias gradient rides on one of the layer's weight-gradient launches)
            tape.defer_wgrad(('w', id(layer), 0), dz, x, gw, 0, bias=None if x2 is not None else _grad_buf(b))
            if x2 is not None:
                tape.defer_wgrad(('w', id(layer), 1), dz, x2, gw, c1, bias=_grad_buf(b))
        if need_dx and c1 <= 4 and cout <= 64 and x2 is None:
            # data gradient onto an image (VGG's first conv): cout -> <=4 channels is the small
            # kernel's shape; its weights are the 180-degree rotated, transposed taps
            tape.add_grad(x, ops.conv3x3_small(dz, packs.get(layer, 'dgrad_small'), None))
        elif need_dx and x2 is None and _prefers_wino(n_, cout, cin, h_, w_):
            tape.add_grad(x, ops.conv3x3_wino(dz, packs.get(layer, 'dgrad_wino'), None, cout, cin, NONE))
        elif need_dx:
            pkd = packs.get(layer, 'dgrad', 0, c1)
            tape.add_grad(x, ops.conv3x3(dz, pkd[0], None, cout, c1, pkd[3], ksplit=None))
        if x2 is not None and need_dx2:
            pkd = packs.get(layer, 'dgrad', c1, cin)
            tape.add_grad(x2, ops.conv3x3(dz, pkd[0], None, cout, cin - c1, pkd[3], ksplit=None))
    tape.record(bwd)
    return y


def resblock(tape, conv1, conv2, x):
    """ResidualBlock (tecogan_nets.py:85-100): out = x + conv2(relu(conv1(x))) with a hand-fused
    backward -- two data-gradient launches per block instead of five:
      dZ1 = relu'(y1) * dgrad2(dOut)      ReLU mask applied in the conv epilogue
      dX  = dgrad1(dZ1) + dOut            the skip connection's gradient rides the residual input
    (the generic tape would run: clone for the skip, dgrad2, act_bwd, dgrad1, axpy)."""
    y1 = conv3x3(None, conv1, x, RELU)
    out = conv3x3(None, conv2, y1, NONE, res=x)
    if tape is None:
        return out
    w1, b1, w2, b2 = conv1.weight, conv1.bias, conv2.weight, conv2.bias
    c = w1.shape[0]

    def bwd():
        g = tape.pop_grad(out)
        if g is None:
            return
        if w2.requires_grad:
            tape.defer_wgrad(('w', id(conv2), 0), g, y1, _grad_buf(w2), 0, bias=_grad_buf(b2))
        pk2 = packs.get(conv2, 'dgrad', 0, w2.shape[1])
        dz1 = ops.conv3x3(g, pk2[0], None, c, c, pk2[3], relu_mask=y1)
        if w1.requires_grad:
            tape.defer_wgrad(('w', id(conv1), 0), dz1, x, _grad_buf(w1), 0, bias=_grad_buf(b1))
        pk1 = packs.get(conv1, 'dgrad', 0, w1.shape[1])
        tape.add_grad(x, ops.conv3x3(dz1, pk1[0], None, c, w1.shape[1], pk1[3], res=g))
    tape.record(bwd)
    return out


# ---------------------------------------------------------------------------
# SRNet's conv_in + residual blocks of one unrolled frame as ONE chained launch
# (tg_srnet_body_fwd / _bwd, csrc/tg_conv3x3_chain.hip), forward and reverse sweep.
# ---------------------------------------------------------------------------
def srnet_body(tape, srnet, lr, tran):
    """conv_in + nb residual blocks (tecogan_nets.py:108-116, :141-143) of one frame: one launch
    forward, one launch for the whole reverse sweep of these 1 + 2*nb layers; the (dZ, X) pairs of
    the weight gradients are deferred exactly as the per-layer nodes defer them."""
    from .. import _lib as L
    n, c_lr, h, w = lr.shape
    layout = 16 if _ChainState.parts(n, h, w) == 4 else 64
    layers, keep, dgp = packs.get(srnet, 'body', layout, c_lr)
    conv_in, nl = layers[0], len(layers)
    nb = (nl - 1) // 2
    c_tran, nf = tran.shape[1], conv_in.cout
    fw = (L.PackedLayer * nl)()
    for i, m in enumerate(layers):
        fw[i].w, fw[i].b = keep[i].data_ptr(), m.bias.data_ptr()
    acts = torch.empty(nl, n, nf, h, w, dtype=torch.float32, device=lr.device)
    flags, err, epoch = _ChainState.buffers(nl + 1, n, h, w, lr.device)
    st = ops._stream()
    L.check(L.lib().tg_srnet_body_fwd(fw, layout, nb, lr.data_ptr(), c_lr, tran.data_ptr(), c_tran, acts.data_ptr(),
                                      n, nf, h, w, flags.data_ptr(), err.data_ptr(), epoch,
                                      _ChainState.poll_limit, st), 'tg_srnet_body_fwd')
    out = acts[nl - 1]
    if tape is None:
        return out
    dz = torch.empty(nl, n, nf, h, w, dtype=torch.float32, device=lr.device)
    tape.reserved[id(out)] = dz[nl - 1]    # the gradient of the body's output lives in the block's last slot

    def bwd():
        g = tape.pop_grad(out)
        tape.reserved.pop(id(out), None)
        if g is None:
            return
        dg = (L.PackedLayer * nl)()
        for i in range(nl):
            dg[i].w = dgp[i].data_ptr()
        if g.data_ptr() != dz[nl - 1].data_ptr():
            dz[nl - 1].copy_(g)   # (a producer that could not write in place)
        d_tran = torch.empty(n, c_tran, h, w, dtype=torch.float32, device=g.device)
        fl, er, ep = _ChainState.buffers(nl + 1, n, h, w, g.device)
        L.check(L.lib().tg_srnet_body_bwd(dg, layout, nb, acts.data_ptr(), dz.data_ptr(), d_tran.data_ptr(),
                                          c_tran, n, nf, h, w, fl.data_ptr(), er.data_ptr(), ep,
                                          _ChainState.poll_limit, ops._stream()),
                'tg_srnet_body_bwd')
        tape.keep.append(dgp)
        if conv_in.weight.requires_grad:
            gw = _grad_buf(conv_in.weight)
            tape.defer_wgrad(('w', id(conv_in), 0), dz[0], lr, gw, 0)
            tape.defer_wgrad(('w', id(conv_in), 1), dz[0], tran, gw, c_lr, bias=_grad_buf(conv_in.bias))
            # the residual-block convs' weight AND bias gradients are taken from the per-frame blocks by
            # one launch when the tape is flushed (conv_in's bias gradient rides on its own launch above)
            tape.defer_body(id(srnet), layers, acts, dz)
        tape.add_grad(tran, d_tran)
    tape.record(bwd)
    tape.keep.append(keep)
    return out


def conv3x3_small(tape, layer, x, act=NONE, up_src=None, up_mode=ops.UP_NONE, up_scale=1, res=None):
    """cout <= 4 head (flow[2] / conv_out).  `up_src` is data (no gradient).  `res` (data as well): the
    already up-sampled residual, added by the small-cout kernel's 4-row form (waves split the input
    channels); shapes it does not take go to the MFMA kernel (3 of 32 output columns used)."""
    w, b = layer.weight, layer.bias
    cout, cin = w.shape[0], w.shape[1]
    if res is not None and cin <= 64 and ops.conv3x3_small_res_ok(x, res):
        y = ops.conv3x3_small(x, w, b, act, res=res)
    elif res is not None and act in (NONE, RELU, LRELU):
        pk, ocb = layer.packed()
        y = ops.conv3x3(x, pk, b, cin, cout, ocb, act, res=res, ksplit=1)
    else:
        y = ops.conv3x3_small(x, w, b, act, up_src=up_src, up_mode=up_mode, up_scale=up_scale)
    if tape is None:
        return y

    def bwd():
        g = tape.pop_grad(y)
        if g is None:
            return
        dz = ops.act_bwd(g, y, act, out=g) if act != NONE else g
        if w.requires_grad:
            tape.defer_wgrad(('w', id(layer), 0), dz, x, _grad_buf(w), 0, bias=_grad_buf(b))
        fuse = id(x) in tape.relu_outputs        # x = relu(...): deliver dZ of that layer directly
        if ops.conv3x3_fewin_ok(dz, cin) and (not fuse or x.data_ptr() % 16 == 0):
            # few channels in, many out: the VALU kernel (the MFMA one pads K = 9 cout to a 72-deep chunk)
            wd = packs.get(layer, 'dgrad_fewin')
            tape.add_grad(x, ops.conv3x3_fewin(dz, wd, relu_mask=x if fuse else None), masked=fuse)
        else:
            pkd = packs.get(layer, 'dgrad', 0, cin)
            tape.add_grad(x, ops.conv3x3(dz, pkd[0], None, cout, cin, pkd[3], ksplit=1,
                                         relu_mask=x if fuse else None), masked=fuse)
    tape.record(bwd)
    return y


# ---------------------------------------------------------------------------
# ConvTranspose2d(k3,s2,p1,op1): forward = sub-pixel phase kernel; backward via
# the space-to-depth embedding (packs._convt_embed).
# ---------------------------------------------------------------------------
def convt3x3s2(tape, layer, x, act=RELU):
    w, b = layer.weight, layer.bias            # (ci, co, 3, 3)
    ci, co = w.shape[:2]
    pk, _ = layer.packed()
    y = ops.convt3x3s2(x, pk, b, co, act)
    if tape is None:
        return y
    if act == RELU:
        tape.relu_outputs.add(id(y))

    def bwd():
        g = tape.pop_grad(y)
        if g is None:
            return
        premasked = act == RELU and id(y) not in tape.unmasked       # every contribution came masked
        dz = ops.act_bwd(g, y, act, out=g) if (act != NONE and not premasked) else g
        fuse = id(x) in tape.relu_outputs
        nx, _, hx, wx = x.shape
        direct = co <= 64 and ci <= 64 and dz.is_contiguous() and x.is_contiguous()
        s = None
        if ops.conv3x3s2_supported(nx, co, ci, hx, wx):
            # small frames: the gradient taken directly as a stride-2 conv of dZ (K = 9 co) -- 11 us
            # instead of 27 us for the 32-chunk phased form on s2d(dZ)
            wk = packs.get(layer, 'convt_dgrad_s2')
            buf = tape.reserved.get(id(x)) if tape.grad(x) is None else None
            tape.add_grad(x, ops.conv3x3s2(dz, wk, co, ci, relu_mask=x if fuse else None, out=buf), masked=fuse)
        else:
            s = ops.space_to_depth(dz, 2)                          # (n, 4co, h, w)
            we = packs.get(layer, 'convt_dgrad_embed')
            if co % 8 == 0:    # phase py = 1 owns tap rows {0, 1}, py = 0 only {1}: 9 of 36 taps are non-zero
                tape.add_grad(x, ops.conv3x3_phased(s, we[0], 4 * co, ci, we[3], 1, co, ops.TAPS_1, ops.TAPS_01,
                                                    relu_mask=x if fuse else None), masked=fuse)
            else:
                tape.add_grad(x, ops.conv3x3(s, we[0], None, 4 * co, ci, we[3], ksplit=1,
                                             relu_mask=x if fuse else None), masked=fuse)
        if w.requires_grad:
            if direct:
                # dW straight from dZ (tg_wgrad3x3_convt_multi): no s2d copy, no embedded gradient to gather back
                tape.defer_wgrad_convt(('ctw', id(layer)), x, dz, _grad_buf(w), _grad_buf(b))
            else:
                if s is None:
                    s = ops.space_to_depth(dz, 2)

                def scatter(ge):                                   # G[ci][(ph,co)][ty][tx]
                    _, inv = _embed_index('convt', ci, co, ge.device)
                    ops.index_gather(ge, inv, out=_grad_buf(w), accumulate=True)
                tape.defer_wgrad_embedded(('ct', id(layer)), x, s, scatter, phased=(co, ops.TAPS_1, ops.TAPS_01))
                tape.defer_bias(_grad_buf(b), dz)
    tape.record(bwd)
    return y


# ---------------------------------------------------------------------------
# Conv2d(k4, s2, p1, no bias) of the discriminator blocks through s2d:
#   2*oy - 1 + ky = 2*(oy + ty - 1) + py     (packs._conv4_embed)
# ---------------------------------------------------------------------------
def direct_conv4():
    """TG_CONV4_DIRECT=0: the embedded form everywhere (lab / tests).  Read per call, so a test can toggle it."""
    return os.environ.get('TG_CONV4_DIRECT', '1') != '0'


def conv4x4s2(tape, holder, x, need_dx=True):
    """holder.weight: (co, ci, 4, 4).  Returns (n, co, h/2, w/2).
    Forward and data gradient run on the direct K = 16 ci kernels (tg_conv4x4s2_fwd / _dgrad, round 4) wherever
    `tg_conv4x4s2_supported` says so: ci, co multiples of 64 and an input 64 or more wide (a multiple of 64) on the
    row-tile kernels, 32 / 16 wide on the small-map kernels (folded pixel tiles, split-K + a summing launch).  Every
    other shape and the weight gradient use the embedding into a phase-masked 3x3 conv on space_to_depth(x, 2) --
    that copy is then made in backward, only when the weights take a gradient."""
    w = holder.weight
    co, ci = w.shape[:2]
    n, _, h_, w_ = x.shape
    direct = direct_conv4() and ops.conv4x4s2_supported(n, ci, co, h_, w_)
    sparse = ci % 8 == 0 and co > 32
    if direct:
        pk4 = packs.get(holder, 'conv4_direct')
        y = ops.conv4x4s2(x, pk4[0], co)
        s_held = [None]
    else:
        s_held = [ops.space_to_depth(x, 2)]
        pk = packs.get(holder, 'conv4_embed')
        # phase coordinate 1 owns tap rows {0, 1}, coordinate 0 rows {1, 2}: 4 of 9 taps per channel
        if sparse:
            y = ops.conv3x3_phased(s_held[0], pk[0], 4 * ci, co, pk[3], 1, ci, ops.TAPS_12, ops.TAPS_01)
        else:
            y = ops.conv3x3(s_held[0], pk[0], None, 4 * ci, co, pk[3])
    if tape is None:
        return y

    def bwd():
        g = tape.pop_grad(y)
        if g is None:
            return
        if w.requires_grad:
            def scatter(ge):
                _, inv = _embed_index('conv4', co, ci, ge.device)
                ops.index_gather(ge, inv, out=_grad_buf(w), accumulate=True)
            s = s_held[0] if s_held[0] is not None else ops.space_to_depth(x, 2)
            tape.defer_wgrad_embedded(('c4', id(holder)), g, s, scatter, phased=(ci, ops.TAPS_12, ops.TAPS_01))
        if need_dx:
            a = tape.act_outputs.get(id(x))
            fuse = a is not None and tape.grad(x) is None
            if direct:
                # x = act(conv(.)): the epilogue applies act'(x) (one pass over the tensor instead of three)
                fuse = fuse and a in (ops.ACT_RELU, ops.ACT_LRELU02)
                gx = ops.conv4x4s2_dgrad(g, pk4[1], ci, act_y=x if fuse else None, act=a if fuse else ops.ACT_NONE)
                tape.add_grad(x, gx, act_applied=fuse)
                return
            pkd = packs.get(holder, 'conv4_dgrad_embed')
            if ci % 64 == 0:    # rot180 taps: coordinate 1 owns rows {1, 2}, coordinate 0 rows {0, 1}
                ds = ops.conv3x3_phased(g, pkd[0], co, 4 * ci, pkd[3], 2, ci, ops.TAPS_01, ops.TAPS_12)
            else:
                ds = ops.conv3x3(g, pkd[0], None, co, 4 * ci, pkd[3], ksplit=1)
            if fuse:
                # x = act(conv(.)): the depth-to-space pass applies act'(x) on the way out (one pass over
                # the HR tensor instead of three)
                gx, fused = ops.depth_to_space(ds, 2, act_y=x, act=a)
                tape.add_grad(x, gx, act_applied=fused)
            else:
                tape.add_grad(x, ops.depth_to_space(ds, 2))
    tape.record(bwd)
    return y


# ---------------------------------------------------------------------------
# pointwise / gather ops
# ---------------------------------------------------------------------------
def maxpool2(tape, x):
    y = ops.maxpool2(x)
    if tape is not None:
        def bwd():
            g = tape.pop_grad(y)
            if g is not None:
                tape.add_grad(x, ops.maxpool2_bwd(x, g))
        tape.record(bwd)
    return y


def upsample(tape, x, scale, up_mode, mul=1.0):
    y = ops.upsample(x, scale, up_mode, mul)
    if tape is not None:
        def bwd():
            g = tape.pop_grad(y)
            if g is not None:
                tape.add_grad(x, ops.upsample_bwd(g, scale, up_mode, mul))
        tape.record(bwd)
    return y


def backward_warp(tape, x, flow, need_dimg=True, need_dflow=True, dflow_out=None, s2d=1):
    """`dflow_out`: a callable returning the buffer the flow gradient is written into (a slice of
    a larger gradient tensor the caller owns, allocated when backward reaches it) instead of
    the gradient being deposited on the tape.  `s2d` > 1: the result is space_to_depth(warp, s2d) -- the
    unroll's warp -> space_to_depth pair (tecogan_nets.py:208-212) as one launch each way."""
    y = ops.backward_warp(x, flow) if s2d == 1 else ops.backward_warp_s2d(x, flow, s2d)
    if tape is not None and (need_dimg or need_dflow):
        def bwd():
            g = tape.pop_grad(y)
            if g is None:
                return
            cur = tape.grad(x) if need_dimg else None
            if cur is not None and cur.is_contiguous() and id(x) not in tape.act_applied:
                # x has a gradient already (its own loss term): the scatter adds into it -- no memset of a new
                # tensor, no accumulation pass
                tape.unmasked.add(id(x))
                _, dflow = ops.backward_warp_bwd(x, flow, g, True, need_dflow,
                                                 dflow_out() if dflow_out is not None else None, dimg_acc=cur, s2d=s2d)
                dimg = None
            else:
                dimg, dflow = ops.backward_warp_bwd(x, flow, g, need_dimg, need_dflow,
                                                    dflow_out() if dflow_out is not None else None, s2d=s2d)
            if need_dimg and dimg is not None:
                tape.add_grad(x, dimg)
            if need_dflow and dflow_out is None:
                tape.add_grad(flow, dflow)
        tape.record(bwd)
    return y


def view(tape, x, shape):
    """Reshape of a contiguous tensor (gradients are keyed by tensor identity, so the
    re-viewed tensor needs its own node)."""
    y = x.view(shape)
    if tape is not None:
        def bwd():
            g = tape.pop_grad(y)
            if g is not None:
                tape.add_grad(x, g.view(x.shape))
        tape.record(bwd)
    return y


def channel_norm(tape, x, mean, std):
    """(x - mean[c]) / std[c]  (vgg_nets.py:29)."""
    y = ops.channel_norm(x, mean, std)
    if tape is not None:
        def bwd():
            g = tape.pop_grad(y)
            if g is not None:
                tape.add_grad(x, ops.channel_norm(g, None, std))
        tape.record(bwd)
    return y


def space_to_depth(tape, x, scale):
    y = ops.space_to_depth(x, scale)
    if tape is not None:
        def bwd():
            g = tape.pop_grad(y)
            if g is not None:
                tape.add_grad(x, ops.depth_to_space(g, scale))
        tape.record(bwd)
    return y


def bn_lrelu(tape, bn, x, need_dx=True, sync=None, groups=1):
    """BatchNorm2d (train mode) + LeakyReLU(0.2); bn holds weight/bias/running stats.
    Under torch.distributed (or sync=True) the statistics are global (SyncBatchNorm).
    groups > 1: x stacks that many INDEPENDENT batches along n (the critic's real + fake pair pass):
    batch statistics per group, the running statistics updated group after group -- exactly what the
    reference's separate passes do -- and, data parallel, ONE collective per layer for all groups."""
    if sync is None:
        sync = _distributed_world() > 1
    n = x.shape[0]
    assert n % groups == 0
    per = n // groups
    if sync:
        y, stats = ops.sync_bn_lrelu_train_fwd_groups(x, groups, bn.weight, bn.bias, bn.running_mean, bn.running_var)
    else:
        y, stats = torch.empty_like(x), []
        for g in range(groups):
            _, mean, invstd = ops.bn_lrelu_train_fwd(x[g * per:(g + 1) * per], bn.weight, bn.bias,
                                                     bn.running_mean, bn.running_var,
                                                     out=y[g * per:(g + 1) * per])
            stats.append((mean, invstd, None))
    for _ in range(groups):
        bn.count_pass() if hasattr(bn, 'count_pass') else bn.num_batches_tracked.add_(1)
    if tape is not None:
        def bwd():
            g_ = tape.pop_grad(y)
            if g_ is None:
                return
            train = bn.weight.requires_grad
            gw = _grad_buf(bn.weight) if train else None
            gb = _grad_buf(bn.bias) if train else None
            if sync:
                dx = ops.sync_bn_lrelu_train_bwd_groups(x, y, g_, groups, bn.weight, stats, gw, gb, need_dx)
            else:
                dx = torch.empty_like(x) if need_dx else None
                for g in range(groups):
                    sl = slice(g * per, (g + 1) * per)
                    ops.bn_lrelu_train_bwd(x[sl], y[sl], g_[sl], bn.weight, stats[g][0], stats[g][1], gw, gb,
                                           need_dx, dx_out=dx[sl] if need_dx else None)
            if need_dx:
                tape.add_grad(x, dx)
        tape.record(bwd)
    return y


def linear1(tape, lin, x, need_dx=True):
    y = ops.linear1_fwd(x, lin.weight, lin.bias)
    if tape is not None:
        def bwd():
            g = tape.pop_grad(y)
            if g is None:
                return
            train = lin.weight.requires_grad
            dx = ops.linear1_bwd(x, lin.weight, g, _grad_buf(lin.weight) if train else None,
                                 _grad_buf(lin.bias) if train else None, need_dx)
            if need_dx:
                tape.add_grad(x, dx)
        tape.record(bwd)
    return y
