"""The one-launch conv bodies at every buffer placement their C ABI admits (KERNELS.md, "Buffer placement", third table):
tg_conv3x3_wino_chain, tg_conv3x3_wino_resident(_ct), tg_conv3x3_chain (both kernels, forward and backward layer
patterns), tg_srnet_body_fwd / _bwd, and the five buffers a caller hands to tg_frnet_step.

The method is that of tests/test_hip_placement.py and tests/test_hip_placement_bwd.py, unchanged: all operands of a launch
live in one Arena whose every other word is a recognisable quiet NaN, the entry points are called through the C ABI with
data_ptr() and explicit strides, n = 2 (the resident launch: 1), every movable operand goes alone to each placement that
applies to it, then all of them together.  What these launches add:

  * a tensor that one layer writes and another reads is ONE operand: its pointer and stride go into every layer struct
    that names it and it moves as a whole -- so "the ping-pong tensor alone at P1" is a case, and with it the launch in
    which ONE misaligned tensor takes every layer of tg_conv3x3_wino_chain off the float2 epilogue;
  * every case runs in two buffer patterns: 'own' gives every layer a destination of its own, so that every
    intermediate reaches memory and is checked against fp64, teacher-forced (the reference of layer i is computed
    from the launch's OWN fp32 input to layer i, read back from the arena); 'srnet' is what production runs, two
    ping-pong tensors with the in-place residual sum (Arena.inout with prefill: the first layer writes them before
    anyone reads them, and finite() still tells a never-written element from a guard read);
  * flag buffers and the resident workspace are destinations of EXACTLY the words the entry's query returns, zeroed once
    per arena (epoch = 1): Arena.check() proves that nothing was written behind them, and the launch's own fault counter
    is read out of them and must be 0 at every placement;
  * the resident launch never writes its intermediate tensors (nor, with the transposed-conv tail, the last layer's y):
    those operands hold a guard pattern of their own as INPUTS, so check() proves them untouched and a read of them
    would show as a NaN in the result.

Every launched placement asserts the return code, Arena.check(), Arena.finite() on every destination, the fault counter,
the fp64 bound of the entry's existing test (1e-5 of the reference's scale for the Winograd launches,
test_conv3x3_winograd_form; relerr <= 2e-5 for the row chain, test_srnet_body_chain_equals_layer_launches; 3e-6 for the
transposed-conv tail, test_winograd_resident_launch_with_transposed_conv_tail), bit-identity with the P0 result, and --
the two Winograd launches -- bit-identity with one tg_conv3x3_wino_fwd launch per layer; the 'srnet' pattern must give
the 'own' pattern's tensors bit for bit.  No form of these kernels sums in another order: the placements choose store
width and addressing only (wino chain: vec_ok on the host; row chain: per layer and image on the device; the
16 x 16 x 4 kernel stores element by element always).

Refusals: a batch stride below one image (TG_E_SHAPE: the `L<i>.<field>@overlap` tags, which hand ONE stride field of
ONE layer struct one float less than an image, the operands at P0 -- one tag per TG_REQUIRE_LAYER_NSTRIDE line of
the two launchers), a last-layer y of the resident launch that is not 8-byte aligned (`<y>@P1`), a tail destination
that is not 16-byte aligned (`ct_y@P1`, `ct_y@P2`) and a workspace that is not 256-byte aligned (`ws@P1`, `ws@P2`), all
TG_E_ARG; each asserts that nothing was written.

tests/test_placement_chain_cpu.py restates the host-side choices and asserts that the tables below, crossed with the
placements, reach both values of each."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from tests.placement import GUARD
from tests.test_hip_placement import (Operand, Case, N, TG_E_ARG, TG_E_SHAPE, rs, al, run_case, ops, lib)   # noqa: F401
from tests.test_hip_placement_bwd import Op

pytestmark = pytest.mark.gpu

POLL_LIMIT = 1 << 21             # what ops.RowChain.run passes
NF = 64

# ======================================================================================================================
# the case tables (plain data; the smallest shapes that still reach each form)
# ======================================================================================================================
# tg_conv3x3_wino_chain: h, w, cin of the first layer, c1 (channels of its first source; None: a single source)
WINO_CHAIN_CASES = [
    (4, 64, 51, 3),      # two full 2 x 32 tiles in x; float2 epilogue at P0, element stores as soon as ONE y / res is odd
    (4, 34, 51, 3),      # a ragged second tile (2 of 32 columns), still float2 at P0
    (3, 33, 51, 3),      # element stores by shape, whatever the placement
    (4, 64, 15, None),   # a 15-channel single-source first layer: one K stage
]
# tg_conv3x3_wino_resident / _ct: h, w (n = 1; each without and with the transposed-conv tail)
WINO_RES_CASES = [
    (8, 24),             # one 8 x 24 block
    (10, 26),            # four blocks, partial at the right and at the bottom
]
# tg_conv3x3_chain, forward and backward layer patterns: h, w.  At n = 2 these are 16 / 20 / 20 tiles: the 16 x 16 x 4
# kernel (tg_conv3x3_chain_supported = 4, pack_layout 16), one store per element at any placement
ROW_CHAIN_CASES = [
    (8, 32),             # one tile in x
    (5, 40),             # two tiles in x, w % 4 == 0
    (5, 37),             # ... ragged, odd width
]
# the larger maps are found by asking tg_conv3x3_chain_supported (w = 32, h counted up): the smallest n = 2 map that
# runs with 2 workgroups per tile (conv3x3_rowchain_kernel<8>: 8-byte stores where y, its stride and h w allow) and
# with 1 (<4>: 16-byte stores).  On the MI355X: (33, 32), the first with 4 * ntile > 256 CUs, and (65, 32), the first
# past half of what the device holds of <8>.  They run at these placements only:
ROW_CHAIN_LARGE_PARTS = (2, 1)
ROW_CHAIN_LARGE_TAGS = ('all@P1', 'all@P3', 'all@P4')
# tg_srnet_body_fwd / _bwd: h, w (nb = 1; no strides in this ABI: bases at P0..P2)
BODY_CASES = [(8, 32), (5, 37)]
# tg_frnet_step, 4 x BD, n = 1: h, w, the body launch asked for.  (8, 8) is the plan's minimum size and runs one launch
# per layer; (16, 48) runs SRNet's body as the resident launch (with the transposed-conv tail) where the device
# supports it -- the plan's switches are read once per process, so that row runs in a child process
FRNET_STEP_CASES = [(8, 8, 'default'), (16, 48, 'resident')]
PATTERNS = ('own', 'srnet')


# ======================================================================================================================
# helpers
# ======================================================================================================================
class CCase(Case):
    """Case plus: only (the tags to run besides P0; None: all), and infos() for the CPU file."""

    def __init__(self, *a, only=None, **kw):
        super().__init__(*a, **kw)
        self.only = only

    def placements(self):
        """(an operand marked alone_only -- the resident workspace, which may not move -- goes to its placements alone,
        where the launcher's refusal is asserted, and stays at P0 in the all@ placements)"""
        stay = {o.name for o in self.operands if getattr(o, 'alone_only', False)}
        out = []
        for t, pl in super().placements():
            if t.startswith('all@'):
                pl = {k: v for k, v in pl.items() if k not in stay}
            if self.only is None or t in self.only:
                out.append((t, pl))
        return out

    def infos(self):
        return [(tag, {o.name: o.resolve(pl.get(o.name, 'P0')) for o in self.operands})
                for tag, pl in [('P0', {})] + self.placements()]


def zeroed(name, words, align=None):
    """A flag buffer / workspace: a destination of exactly `words` 32-bit words that starts as zeros (zeroed once, as
    the ABI asks), optionally on an alignment of its own.  Its content is part of the result: the flags and the fault
    counter of a launch are the same at every placement."""
    o = Op(name, 'out', shape=(int(words),))
    o.zero = True
    if align:
        o.align = align
    return o


def untouchable(name, shape, movable=False):
    """An operand the launch is handed but may neither read nor write: it holds a quiet NaN pattern of its own as an
    INPUT, so Arena.check() proves it bit for bit afterwards and a value read from it would turn the result NaN."""
    data = torch.full(shape, GUARD | 0xEE, dtype=torch.int32).view(torch.float32)
    return Op(name, 'in' if movable else 'fixed', data)


def ints(t):
    return t.contiguous().view(torch.int32)


def same_bits_as(name, want, what=None):
    """verify(): output `name` is `want` bit for bit."""
    def verify(outs):
        assert outs[name].shape == want.shape, (outs[name].shape, want.shape)
        return [(what or f'{name} (elements that differ)', float((ints(outs[name]) != ints(want)).sum()), 0.0)]
    return verify


def counter_is_zero(name, index):
    """verify(): the launch's own fault counter, int `index` of the zeroed destination `name`."""
    def verify(outs):
        return [('faults', float(ints(outs[name])[index].item()), 0.0)]
    return verify


def flags_all_set(name, count, epoch=1):
    def verify(outs):
        return [('flags not set', float((ints(outs[name])[:count] != epoch).sum()), 0.0)]
    return verify


def every(*verifiers):
    return lambda outs: [r for v in verifiers for r in v(outs)]


def act_ref(t, act):
    return torch.relu(t) if act == 1 else t


def layer_ref(x, wt, b, act, res=None, mask=None, transposed=False):
    """fp64: mask > 0 ? act(conv(x) + b) + res : 0 (transposed: the data gradient of the layer with weights wt)."""
    if transposed:
        r = F.conv_transpose2d(x.double(), wt.double(), None, padding=1)
    else:
        r = F.conv2d(x.double(), wt.double(), None if b is None else b.double(), padding=1)
    r = act_ref(r, act)
    if res is not None:
        r = r + res.double()
    if mask is not None:
        r = torch.where(mask.double() > 0, r, torch.zeros_like(r))
    return r


def teacher_forced(name, ref_of, tol, absolute_cap=False):
    """verify(): output `name` against ref_of(outs), the fp64 layer applied to the launch's own inputs to it; the error
    relative to the reference's scale (absolute_cap: to min(1, scale), which also keeps the absolute 1e-5 of
    test_conv3x3_winograd_form)."""
    def verify(outs):
        ref = ref_of(outs)
        scale = ref.abs().max().item() + 1e-30
        if absolute_cap:
            scale = min(1.0, scale)
        return [(name, (outs[name].double() - ref).abs().max().item() / scale, tol)]
    return verify


def body_weights(cin0):
    """conv_in (cin0 -> 64) and one residual block, as in the existing tables: rs(-1, 1) / (3 sqrt(cin))."""
    ws = [rs(20, (NF, cin0, 3, 3)) / (3.0 * cin0 ** 0.5), rs(21, (NF, NF, 3, 3)) / (3.0 * 8), rs(22, (NF, NF, 3, 3)) / (3.0 * 8)]
    bs = [rs(30 + i, (NF,), -0.5, 0.5) for i in range(3)]
    return ws, bs


def body_inputs(n, cin0, c1, h, w):
    x = rs(1, (n, cin0, h, w))
    return (x[:, :c1].contiguous(), x[:, c1:].contiguous()) if c1 else (x, None)


def overlap_cases(case, spec):
    """One refusal case per (layer, strided field) of the layer table `spec`: the operands at P0, THAT stride of THAT
    layer struct one float short of an image (the other structs that name the tensor keep the true stride, so each
    case stands on one TG_REQUIRE_LAYER_NSTRIDE line).  TG_E_SHAPE with "layer i: <field>_nstride", nothing written."""
    out = []
    for i, d in enumerate(spec):
        for f in ('x', 'x2', 'res', 'mask', 'y'):
            if not d.get(f):
                continue

            def call(lib, p, s, i=i, f=f):
                rc = case.call(lib, p, s, short=(i, f))
                msg = lib.tg_last_error_string().decode()
                assert rc != TG_E_SHAPE or f'layer {i}: {f}_nstride' in msg, msg
                return rc
            out.append(CCase(f'{case.id} L{i}.{f}@overlap', case.operands, call, case.verify,
                             expect=lambda info: TG_E_SHAPE, only=()))
    return out


def stride_of(s, name, short, i, field):
    return s[name] - (1 if short == (i, field) else 0)


# ======================================================================================================================
# tg_conv3x3_wino_chain
# ======================================================================================================================
def wino_spec(pattern, dual):
    """The three layers as operand NAMES: conv_in (ReLU) -> conv1 (ReLU) -> conv2 + res."""
    a, b, c = ('t0', 't1', 't2') if pattern == 'own' else ('A', 'B', 'A')
    return [dict(x='x', x2='x2' if dual else None, u='u0', bias='b0', res=None, y=a, act=1),
            dict(x=a, x2=None, u='u1', bias='b1', res=None, y=b, act=1),
            dict(x=b, x2=None, u='u2', bias='b2', res=a, y=c, act=0)]


def wino_struct(L, spec, p, s, cin0, c1, short=None):
    arr = (L.WinoLayer * len(spec))()
    for i, (a, d) in enumerate(zip(arr, spec)):
        a.x, a.x_nstride = p[d['x']], stride_of(s, d['x'], short, i, 'x')
        if d['x2']:
            a.x2, a.x2_nstride = p[d['x2']], stride_of(s, d['x2'], short, i, 'x2')
        if d['res']:
            a.res, a.res_nstride = p[d['res']], stride_of(s, d['res'], short, i, 'res')
        a.u_packed, a.bias, a.y, a.y_nstride = p[d['u']], p[d['bias']], p[d['y']], stride_of(s, d['y'], short, i, 'y')
        a.cin, a.c1, a.act = (cin0, c1 or cin0, d['act']) if i == 0 else (NF, NF, d['act'])
    return arr


def wino_operands(n, h, w, cin0, c1, pattern, packed, strided=True, movable_mid=True):
    """x, x2, the packed weights and biases (fixed) and the activation tensors of the pattern.  packed: the three U
    tensors (CPU copies), or None on a machine without a GPU (the CPU file reads placements only)."""
    x, x2 = body_inputs(n, cin0, c1, h, w)
    ws, bs = body_weights(cin0)
    opers = [Op('x', 'in', x, strided=strided)] + ([Op('x2', 'in', x2, strided=strided)] if c1 else [])
    opers += [Op(f'u{i}', 'fixed', packed[i] if packed else torch.zeros(4)) for i in range(3)]
    opers += [Op(f'b{i}', 'fixed', bs[i]) for i in range(3)]
    shape = (n, NF, h, w)
    if pattern == 'own':
        opers += [Op(k, 'out', shape=shape, strided=strided, p5=strided) for k in ('t0', 't1', 't2')]
    else:
        opers += [Op(k, 'inout', torch.zeros(shape), prefill=True, strided=strided, p5=strided) for k in ('A', 'B')]
    return opers, (x, x2, ws, bs)


def wino_per_layer(ops, x, x2, ws, bs, cin0):
    """One tg_conv3x3_wino_fwd launch per layer on torch's own allocations: (packed U on the CPU, [t0, t1, t2])."""
    us = [ops.pack_conv3x3_wino(wt.cuda()) for wt in ws]
    b = [t.cuda() for t in bs]
    t0 = ops.conv3x3_wino(x.cuda(), us[0], b[0], cin0, NF, 1, x2=None if x2 is None else x2.cuda())
    t1 = ops.conv3x3_wino(t0, us[1], b[1], NF, NF, 1)
    t2 = ops.conv3x3_wino(t1, us[2], b[2], NF, NF, 0, res=t0)
    torch.cuda.synchronize()
    return [u.cpu() for u in us], [t.cpu() for t in (t0, t1, t2)]


def wino_teacher(x, x2, ws, bs):
    """The per-layer fp64 bounds of the 'own' pattern: each layer from the launch's own input to it."""
    xin = x if x2 is None else torch.cat([x, x2], 1)
    return every(teacher_forced('t0', lambda o: layer_ref(xin, ws[0], bs[0], 1), 1e-5, True),
                 teacher_forced('t1', lambda o: layer_ref(o['t0'], ws[1], bs[1], 1), 1e-5, True),
                 teacher_forced('t2', lambda o: layer_ref(o['t1'], ws[2], bs[2], 0, res=o['t0']), 1e-5, True))


def wino_chain_case(lib, h, w, cin0, c1, pattern, packed=None, want=None):
    from tecogan_pytorch_amd import _lib as L
    opers, (x, x2, ws, bs) = wino_operands(N, h, w, cin0, c1, pattern, packed)
    nints = lib.tg_conv3x3_wino_chain_flag_ints(3, N, h, w)
    opers.append(zeroed('flags', nints))
    spec = wino_spec(pattern, bool(c1))

    def call(lib, p, s, short=None):
        return lib.tg_conv3x3_wino_chain(wino_struct(L, spec, p, s, cin0, c1, short), 3, N, NF, h, w, p['flags'], 1, None)
    checks = [counter_is_zero('flags', nints - 16), flags_all_set('flags', nints - 16)]
    if want is not None:
        names = ('t0', 't1', 't2') if pattern == 'own' else (None, 'B', 'A')
        checks += [same_bits_as(k, t, f'{k} (elements that differ from the per-layer launches)') for k, t in zip(names, want) if k]
    if pattern == 'own':
        checks.append(wino_teacher(x, x2, ws, bs))
    case = CCase(f'conv3x3_wino_chain {cin0}->64 {h}x{w} c1={c1} {pattern}', opers, call, every(*checks))
    case.spec = spec
    return case


@pytest.mark.parametrize('pattern', PATTERNS)
@pytest.mark.parametrize('h,w,cin0,c1', WINO_CHAIN_CASES)
def test_wino_chain_placements(ops, lib, h, w, cin0, c1, pattern):
    """tg_conv3x3_wino_chain accepts every placement.  vec_ok is ONE choice for the launch: the float2 epilogue (and
    the float2 residual prefetch) runs while w and h w are even and y / res of EVERY layer are 8-byte aligned with
    even strides -- P2 and P4 keep it, one tensor at P1 or P3 (or at P5 where 3 h w is odd) turns every layer to
    element stores; x / x2 never matter.  Same inverse transform and epilogue order in both: bit-identical, and
    identical to one tg_conv3x3_wino_fwd launch per layer."""
    x, x2 = body_inputs(N, cin0, c1, h, w)
    ws, bs = body_weights(cin0)
    packed, want = wino_per_layer(ops, x, x2, ws, bs, cin0)
    case = wino_chain_case(lib, h, w, cin0, c1, pattern, packed, want)
    run_case(lib, case)
    if pattern == 'own' and (h, w) == WINO_CHAIN_CASES[0][:2]:
        for c in overlap_cases(case, case.spec):
            run_case(lib, c)


# ======================================================================================================================
# tg_conv3x3_wino_resident / tg_conv3x3_wino_resident_ct
# ======================================================================================================================
def wino_res_case(lib, h, w, pattern, tail, packed=None, want=None, ct=None):
    """n = 1: only bases move (x, x2, the last layer's y, the tail's y; the workspace, whose 256-byte alignment the
    launcher insists on).  The intermediate tensors -- and with the tail the last layer's y -- are never written."""
    from tecogan_pytorch_amd import _lib as L
    cin0, c1 = 51, 3
    opers, (x, x2, ws, bs) = wino_operands(1, h, w, cin0, c1, 'own', packed, strided=False)
    spec = wino_spec(pattern, True)
    last = spec[-1]['y']
    mids = sorted({d['y'] for d in spec} - {last})
    opers = [o for o in opers if o.name not in ('t0', 't1', 't2')]
    opers += [untouchable(k, (1, NF, h, w)) for k in mids]
    opers.append(untouchable(last, (1, NF, h, w), movable=True) if tail else Op(last, 'out', shape=(1, NF, h, w)))
    nwords = lib.tg_conv3x3_wino_resident_ws_bytes(h, w) // 4
    opers.append(zeroed('ws', nwords, align=64))
    opers[-1].alone_only = True
    if tail:
        opers += [Op('ct_u', 'fixed', ct['u'] if ct else torch.zeros(4)), Op('ct_b', 'fixed', ct['b'] if ct else torch.zeros(NF)),
                  Op('ct_y', 'out', shape=(1, NF, 2 * h, 2 * w))]

    def call(lib, p, s):
        arr = wino_struct(L, spec, p, s, cin0, c1)
        if not tail:
            return lib.tg_conv3x3_wino_resident(arr, 3, NF, h, w, p['ws'], 1, None)
        c = L.WresConvT(p['ct_u'], p['ct_b'], p['ct_y'], 1)
        return lib.tg_conv3x3_wino_resident_ct(arr, 3, NF, h, w, p['ws'], 1, ctypes.byref(c), None)

    def expect(info):
        ok = info['ws'][0] == 0 and info[last][0] % 2 == 0 and (not tail or info['ct_y'][0] % 4 == 0)
        return 0 if ok else TG_E_ARG
    checks = [counter_is_zero('ws', nwords - 64)]
    if want is not None and not tail:
        checks.append(same_bits_as(last, want[2], f'{last} (elements that differ from the per-layer launches)'))
    if ct and tail:
        ref = torch.relu(F.conv_transpose2d(want[2].double(), ct['w'].double(), ct['b'].double(), 2, 1, 1))
        scale = ref.abs().max().item()
        checks.append(lambda outs: [('ct_y', (outs['ct_y'].double() - ref).abs().max().item() / scale, 3e-6),
                                    ('ct_y vs tg_convt3x3s2_fwd', (outs['ct_y'].double() - ct['gpu'].double()).abs().max().item() / scale, 3e-6)])
    return CCase(f'conv3x3_wino_resident{"_ct" if tail else ""} {h}x{w} {pattern}', opers, call, every(*checks), expect=expect)


@pytest.mark.parametrize('tail', [False, True])
@pytest.mark.parametrize('pattern', PATTERNS)
@pytest.mark.parametrize('h,w', WINO_RES_CASES)
def test_wino_resident_placements(ops, lib, h, w, pattern, tail):
    """tg_conv3x3_wino_resident(_ct): x / x2 are read element by element through bounded descriptors at any base.  The
    last layer's y leaves as float2 rows: the launcher checked only that it was non-null and now wants it 8-byte
    aligned (TG_E_ARG at P1, with and without the tail: one rule); the tail's y is 16-byte aligned (P1 and P2 are
    TG_E_ARG), the workspace 256-byte aligned.  The result is that of one tg_conv3x3_wino_fwd launch per layer, bit
    for bit; the intermediate tensors (and with the tail the last y) keep their pattern."""
    if not lib.tg_conv3x3_wino_resident_supported(1, NF, h, w):
        pytest.skip(f'tg_conv3x3_wino_resident_supported(1, 64, {h}, {w}) = 0 on this device')
    x, x2 = body_inputs(1, 51, 3, h, w)
    ws, bs = body_weights(51)
    packed, want = wino_per_layer(ops, x, x2, ws, bs, 51)
    ct = None
    if tail:
        wt, bt = rs(40, (NF, NF, 3, 3)) / (1.5 * 8), rs(41, (NF,), -0.5, 0.5)
        pk = ops.pack_conv3x3(wt.cuda(), transposed=True)[0]
        ct = dict(w=wt, b=bt, u=ops.pack_wres_convt(wt.cuda()).cpu(),
                  gpu=ops.convt3x3s2(want[2].cuda(), pk, bt.cuda(), NF, 1).cpu())
    run_case(lib, wino_res_case(lib, h, w, pattern, tail, packed, want, ct))


# ======================================================================================================================
# tg_conv3x3_chain: conv3x3_rowchain16_kernel (4 workgroups per tile), conv3x3_rowchain_kernel<8> (2) and <4> (1)
# ======================================================================================================================
def smallest_map(lib, parts):
    """The smallest n = 2, w = 32 map tg_conv3x3_chain_supported runs with `parts` workgroups per tile (asked, not
    restated); None where this device has none below 400 rows."""
    for h in range(1, 400):
        if lib.tg_conv3x3_chain_supported(N, h, 32, NF) == parts:
            return h, 32
    return None


def chain_struct(L, spec, p, s, short=None):
    arr = (L.ChainLayer * len(spec))()
    for i, (a, d) in enumerate(zip(arr, spec)):
        a.x, a.x_nstride, a.w_packed = p[d['x']], stride_of(s, d['x'], short, i, 'x'), p[d['w']]
        a.y, a.y_nstride = p[d['y']], stride_of(s, d['y'], short, i, 'y')
        for k, ptr, ns in (('x2', 'x2', 'x2_nstride'), ('res', 'res', 'res_nstride'), ('mask', 'relu_mask', 'mask_nstride')):
            if d.get(k):
                setattr(a, ptr, p[d[k]])
                setattr(a, ns, stride_of(s, d[k], short, i, k))
        if d.get('bias'):
            a.bias = p[d['bias']]
        a.c1, a.cin, a.cout, a.act = d['c1'], d['cin'], d['cout'], d['act']
    return arr


C_LR, C_TRAN = 3, 48


def row_chain_case(lib, h, w, direction, pattern, parts=None, packed=None, only=None, share=None):
    """direction 'fwd': conv_in with two sources + one block (x2, bias, res, ReLU).  'bwd': the layers tg_srnet_body_bwd
    builds for nb = 1 -- act NONE, relu_mask from a fixed input tensor, res, and a last layer with cout = 48 into an
    (n, 48, h, w) destination.  share: a dict the 'own' case leaves its P0 tensors in and the 'srnet' case of the same
    shape compares with."""
    from tecogan_pytorch_amd import _lib as L
    cin0 = C_LR + C_TRAN
    ws, bs = body_weights(cin0)
    shape = (N, NF, h, w)
    wnames = ['w0', 'w1', 'w2']
    opers = [Op(k, 'fixed', packed[i] if packed else torch.zeros(4)) for i, k in enumerate(wnames)]
    if direction == 'fwd':
        x, x2 = body_inputs(N, cin0, C_LR, h, w)
        a, b, c = ('t0', 't1', 't2') if pattern == 'own' else ('A', 'B', 'A')
        opers += [Op('x', 'in', x, strided=True), Op('x2', 'in', x2, strided=True)] + [Op(f'b{i}', 'fixed', bs[i]) for i in range(3)]
        if pattern == 'own':
            opers += [Op(k, 'out', shape=shape, strided=True, p5=True) for k in ('t0', 't1', 't2')]
        else:
            opers += [Op(k, 'inout', torch.zeros(shape), prefill=True, strided=True, p5=True) for k in ('A', 'B')]
        spec = [dict(x='x', x2='x2', w='w0', bias='b0', y=a, c1=C_LR, cin=cin0, cout=NF, act=1),
                dict(x=a, w='w1', bias='b1', y=b, c1=NF, cin=NF, cout=NF, act=1),
                dict(x=b, w='w2', bias='b2', res=a, y=c, c1=NF, cin=NF, cout=NF, act=0)]
        xin = torch.cat([x, x2], 1)
        finals = {'own': ('t1', 't2'), 'srnet': ('B', 'A')}[pattern]
        teacher = [teacher_forced('t0', lambda o: layer_ref(xin, ws[0], bs[0], 1), 2e-5),
                   teacher_forced('t1', lambda o: layer_ref(o['t0'], ws[1], bs[1], 1), 2e-5),
                   teacher_forced('t2', lambda o: layer_ref(o['t1'], ws[2], bs[2], 0, res=o['t0']), 2e-5)]
    else:
        g, m1, m0 = rs(2, shape), rs(3, shape), rs(4, shape)
        # 'own' is what tg_srnet_body_bwd runs (every dz its own tensor); 'srnet' is the forward's reuse turned round:
        # the residual sum lands in place on the incoming gradient, which the last layer then reads
        d1, d0 = ('dz1', 'dz0') if pattern == 'own' else ('B', 'g')
        opers += [Op('g', 'in', g, strided=True) if pattern == 'own' else Op('g', 'inout', g, strided=True, p5=True),
                  Op('m1', 'in', m1, strided=True), Op('m0', 'in', m0, strided=True)]
        if pattern == 'own':
            opers += [Op(k, 'out', shape=shape, strided=True, p5=True) for k in ('dz1', 'dz0')]
        else:
            opers.append(Op('B', 'inout', torch.zeros(shape), prefill=True, strided=True, p5=True))
        opers.append(Op('d_tran', 'out', shape=(N, C_TRAN, h, w), strided=True, p5=True))
        spec = [dict(x='g', w='w2', mask='m1', y=d1, c1=NF, cin=NF, cout=NF, act=0),
                dict(x=d1, w='w1', res='g', mask='m0', y=d0, c1=NF, cin=NF, cout=NF, act=0),
                dict(x=d0, w='w0', y='d_tran', c1=NF, cin=NF, cout=C_TRAN, act=0)]
        finals = {'own': ('dz1', 'dz0', 'd_tran'), 'srnet': ('B', 'g', 'd_tran')}[pattern]
        w_in = ws[0][:, C_LR:].contiguous()
        teacher = [teacher_forced('dz1', lambda o: layer_ref(g, ws[2], None, 0, mask=m1, transposed=True), 2e-5),
                   teacher_forced('dz0', lambda o: layer_ref(o['dz1'], ws[1], None, 0, res=g, mask=m0, transposed=True), 2e-5),
                   teacher_forced('d_tran', lambda o: layer_ref(o['dz0'], w_in, None, 0, transposed=True), 2e-5)]
    nints = lib.tg_conv3x3_chain_flag_ints(3, N, h, w)
    opers.append(zeroed('flags', nints + 16))              # + the err ints, as ops.RowChain allocates them
    layout = 16 if parts == 4 else 64

    def call(lib, p, s, short=None):
        return lib.tg_conv3x3_chain(chain_struct(L, spec, p, s, short), 3, N, h, w, layout, p['flags'], p['flags'] + 4 * nints,
                                    1, POLL_LIMIT, None)
    nflags = 3 * N * h * ((w + 31) // 32) * (parts or 4)
    checks = [counter_is_zero('flags', nints), flags_all_set('flags', nflags)]
    if pattern == 'own':
        checks += teacher
        if share is not None:
            def keep(outs):
                share.setdefault('own', {k: outs[k].clone() for k in finals})
                return []
            checks.append(keep)
    elif share is not None:
        own_names = {'fwd': ('t1', 't2'), 'bwd': ('dz1', 'dz0', 'd_tran')}[direction]
        checks += [same_bits_as(k, share['own'][o], f'{k} (elements that differ from the own-destination pattern)')
                   for k, o in zip(finals, own_names)]
    case = CCase(f'conv3x3_chain {direction} {h}x{w} parts={parts} {pattern}', opers, call, every(*checks), only=only)
    case.spec = spec
    return case


def chain_packs(ops, direction, layout):
    cin0 = C_LR + C_TRAN
    ws, _ = body_weights(cin0)
    dev = [t.cuda() for t in ws]
    if direction == 'fwd':
        items = [(dev[0], 0, cin0, 0), (dev[1], 0, NF, 0), (dev[2], 0, NF, 0)]
    else:       # (w0: conv_in's data gradient restricted to the warped-frame channels [3, 51))
        items = [(dev[0], C_LR, C_TRAN, 2), (dev[1], 0, NF, 2), (dev[2], 0, NF, 2)]
    out = [t.cpu() for t in ops.chain_pack(items, layout)]
    torch.cuda.synchronize()
    return out


PARTS_REACHED = set()


def run_row_chain(ops, lib, h, w, direction, only=None, overlaps=False):
    parts = lib.tg_conv3x3_chain_supported(N, h, w, NF)
    assert parts in (1, 2, 4), f'tg_conv3x3_chain_supported({N}, {h}, {w}, 64) = {parts}'
    PARTS_REACHED.add(parts)
    packed = chain_packs(ops, direction, 16 if parts == 4 else 64)
    share = {}
    for pattern in PATTERNS:
        case = row_chain_case(lib, h, w, direction, pattern, parts, packed, only, share)
        run_case(lib, case)
        if overlaps and pattern == 'own':
            for c in overlap_cases(case, case.spec):
                run_case(lib, c)
    return parts


@pytest.mark.parametrize('direction', ['fwd', 'bwd'])
@pytest.mark.parametrize('h,w', ROW_CHAIN_CASES)
def test_row_chain_placements(ops, lib, h, w, direction):
    """tg_conv3x3_chain at the sizes of the 16 x 16 x 4 kernel: every placement is accepted; x / x2 through 4-byte
    buffer loads bounded per image, res with agent-scope loads behind layer 0 and plain ones in it, relu_mask plain,
    y one bounded 4-byte agent-scope store per element.  Both buffer patterns, bit-identical to P0 and to each other."""
    assert run_row_chain(ops, lib, h, w, direction, overlaps=(h, w) == ROW_CHAIN_CASES[0]) == 4


@pytest.mark.parametrize('direction', ['fwd', 'bwd'])
@pytest.mark.parametrize('parts', ROW_CHAIN_LARGE_PARTS)
def test_row_chain_placements_of_the_32x32x2_kernels(ops, lib, parts, direction):
    """conv3x3_rowchain_kernel<8> (2 workgroups per tile) and <4> (1): the store form is chosen per layer and image on
    the device -- 8- / 16-byte bounded stores while w % 2 | 4 == 0, the image's y is 16-byte aligned, h w % 4 == 0 and
    y_nstride % 4 == 0.  all@P1 takes every layer to element stores by pointer, all@P3 by stride, all@P4 none."""
    hw = smallest_map(lib, parts)
    assert hw is not None, f'no n = 2, w = 32 map runs with {parts} workgroup(s) per tile on this device'
    assert run_row_chain(ops, lib, hw[0], hw[1], direction, only=ROW_CHAIN_LARGE_TAGS) == parts


def test_row_chain_tables_reach_every_kernel(lib):
    """The set of tg_conv3x3_chain_supported values over the tables above (asked of the device, independent of which
    tests of this file ran)."""
    got = {lib.tg_conv3x3_chain_supported(N, h, w, NF) for h, w in ROW_CHAIN_CASES}
    got |= {lib.tg_conv3x3_chain_supported(N, *hw, NF) for hw in map(lambda p: smallest_map(lib, p), ROW_CHAIN_LARGE_PARTS) if hw}
    assert got == {1, 2, 4}, got
    assert lib.tg_conv3x3_chain_supported(N, 36, 32, NF) == 2            # 4 * 72 tiles > 256 CUs


# ======================================================================================================================
# tg_srnet_body_fwd / tg_srnet_body_bwd
# ======================================================================================================================
def body_case(lib, h, w, direction, parts=None, packed=None, acts=None):
    """nb = 1.  The packed blocks are ONE operand each -- acts and dz hold 1 + 2 nb tensors (n, nf, h, w) back to back --
    and only their bases move (P0..P2: no strides in this ABI).  dz[2 nb] is the caller's input, the rest of dz is
    written: Arena.inout with the writable mask over the tensors.  acts: the forward result the sweep is driven by."""
    from tecogan_pytorch_amd import _lib as L
    cin0 = C_LR + C_TRAN
    ws, bs = body_weights(cin0)
    hw = h * w
    opers = [Op(f'w{i}', 'fixed', packed[i] if packed else torch.zeros(4)) for i in range(3)]
    layout = 16 if parts == 4 else 64
    nints = lib.tg_conv3x3_chain_flag_ints(3, N, h, w)
    if direction == 'fwd':
        lr, tran = body_inputs(N, cin0, C_LR, h, w)
        opers += [Op(f'b{i}', 'fixed', bs[i]) for i in range(3)]
        opers += [Op('lr', 'in', lr), Op('tran', 'in', tran), Op('acts', 'out', shape=(3 * N, NF, h, w))]

        def call(lib, p, s):
            pl = (L.PackedLayer * 3)(*[L.PackedLayer(p[f'w{i}'], p[f'b{i}']) for i in range(3)])
            return lib.tg_srnet_body_fwd(pl, layout, 1, p['lr'], C_LR, p['tran'], C_TRAN, p['acts'], N, NF, h, w, p['flags'],
                                         p['flags'] + 4 * nints, 1, POLL_LIMIT, None)
        xin = torch.cat([lr, tran], 1)

        def ref_of(i):
            def f(o):
                a = o['acts'].reshape(3, N, NF, h, w)
                return [layer_ref(xin, ws[0], bs[0], 1), layer_ref(a[0], ws[1], bs[1], 1),
                        layer_ref(a[1], ws[2], bs[2], 0, res=a[0])][i]
            return f

        def part(i):
            def verify(outs):
                got = outs['acts'].reshape(3, N, NF, h, w)[i].double()
                ref = ref_of(i)(outs)
                return [(f'acts[{i}]', (got - ref).abs().max().item() / (ref.abs().max().item() + 1e-30), 2e-5)]
            return verify
        checks = [part(i) for i in range(3)]
    else:
        g = rs(2, (N, NF, h, w))
        dz0 = torch.zeros(3, N, NF, h, w)
        dz0[2] = g
        writable = torch.zeros(3, 1, 1, 1, 1, dtype=torch.bool)
        writable[:2] = True
        a = acts.reshape(3, N, NF, h, w)
        opers += [Op('acts', 'in', acts.reshape(3 * N, NF, h, w)),
                  Op('dz', 'inout', dz0.reshape(3 * N, NF, h, w), writable=writable.expand(3, N, 1, 1, 1).reshape(3 * N, 1, 1, 1),
                     prefill=True),
                  Op('d_tran', 'out', shape=(N, C_TRAN, h, w))]

        def call(lib, p, s):
            pl = (L.PackedLayer * 3)(*[L.PackedLayer(p[f'w{i}'], None) for i in range(3)])
            return lib.tg_srnet_body_bwd(pl, layout, 1, p['acts'], p['dz'], p['d_tran'], C_TRAN, N, NF, h, w, p['flags'],
                                         p['flags'] + 4 * nints, 1, POLL_LIMIT, None)
        # the fp64 sweep of test_srnet_body_chain_equals_layer_launches, driven by the masks of the forward result
        # (so that no sign is decided twice), teacher-forced layer by layer
        w_in = ws[0][:, C_LR:].contiguous()

        def sweep(outs):
            d = outs['dz'].reshape(3, N, NF, h, w)
            r1 = layer_ref(g, ws[2], None, 0, mask=a[1], transposed=True)
            r0 = layer_ref(d[1], ws[1], None, 0, res=g, mask=a[0], transposed=True)
            rt = layer_ref(d[0], w_in, None, 0, transposed=True)
            rel_ = lambda got, ref: (got.double() - ref).abs().max().item() / (ref.abs().max().item() + 1e-30)   # noqa: E731
            return [('dz[1]', rel_(d[1], r1), 2e-5), ('dz[0]', rel_(d[0], r0), 2e-5), ('d_tran', rel_(outs['d_tran'], rt), 2e-5),
                    ('dz[2] (elements changed)', float((ints(d[2]) != ints(g)).sum()), 0.0)]
        checks = [sweep]
    opers.append(zeroed('flags', nints + 16))
    checks += [counter_is_zero('flags', nints)]
    only = [f'{o.name}@{p}' for o in opers if o.kind != 'fixed' for p in ('P1', 'P2')] + ['all@P1', 'all@P2']
    return CCase(f'srnet_body_{direction} nb=1 {h}x{w} parts={parts}', opers, call, every(*checks), only=only)


@pytest.mark.parametrize('h,w', BODY_CASES)
def test_srnet_body_placements(ops, lib, h, w):
    """tg_srnet_body_fwd / _bwd build their tg_chain_layer arrays from packed blocks and hand them to tg_conv3x3_chain:
    at these sizes the 16 x 16 x 4 kernel, which reads and writes element by element -- every 4-byte aligned base of lr,
    tran, acts, dz and d_tran is accepted.  The sweep is driven by the acts the forward launch produced at P0."""
    parts = lib.tg_conv3x3_chain_supported(N, h, w, NF)
    assert parts == 4
    fwd = body_case(lib, h, w, 'fwd', parts, chain_packs(ops, 'fwd', 16))
    kept = {}
    verify = fwd.verify

    def verify_and_keep(outs):
        kept.setdefault('acts', outs['acts'].clone())
        return verify(outs)
    fwd.verify = verify_and_keep
    run_case(lib, fwd)
    run_case(lib, body_case(lib, h, w, 'bwd', parts, chain_packs(ops, 'bwd', 16), kept['acts']))


# ======================================================================================================================
# tg_frnet_step: the caller's five buffers
# ======================================================================================================================
def frnet_step_case(h, w, handle=None, data=None, stream=None):
    """lr_curr, lr_prev (1, 3, h, w), hr_prev, hr_out (1, 3, 4h, 4w) and u8_out (4h, 4w, 3) uint8, carried as whole 32-bit
    words.  Everything else the frame touches is the plan's own workspace."""
    H, W = 4 * h, 4 * w
    lr_curr, lr_prev, hr_prev = data if data else (torch.zeros(1, 3, h, w), torch.zeros(1, 3, h, w), torch.zeros(1, 3, H, W))
    opers = [Op('lr_curr', 'in', lr_curr), Op('lr_prev', 'in', lr_prev), Op('hr_prev', 'in', hr_prev),
             Op('hr_out', 'out', shape=(1, 3, H, W)), Op('u8_out', 'scratch', shape=(H * W * 3 // 4,))]

    def call(lib, p, s):
        return lib.tg_frnet_step(handle, p['lr_curr'], p['lr_prev'], p['hr_prev'], p['hr_out'], p['u8_out'], stream)
    return CCase(f'frnet_step 4xBD {h}x{w}', opers, call, None)


def frnet_step_run(h, w, body):
    """One frame at P0, then each of the caller's buffers alone at P1 and P2, then all together.  The caller's pointers
    reach tg_conv3x3_fwd (lr_curr / lr_prev as the two sources of FNet's first layer), tg_flowup_warp_s2d_fwd (hr_prev),
    the first layer of SRNet's body (lr_curr: tg_conv3x3_fwd, or the resident launch's bounded loads) and
    tg_convout_tail (lr_curr as the bicubic source, hr_out, u8_out): all of them take any 4-byte aligned base, the tail
    with its four-pixel form only while hr_out is 16-byte aligned (and u8_out 4-byte aligned) and the same sums
    otherwise.  hr_out: finite, within smoke()'s 1e-4 of the CPU oracle at P0, bit-identical to P0 everywhere; u8_out:
    what tg_quantize_u8_hwc makes of that hr_out, bit for bit; the plan's fault counter 0."""
    import numpy as np
    from oracle import tecogan_oracle as O
    from procedural_weights import generator_state_dict, smooth_clip
    from tecogan_pytorch_amd import _lib as L
    import tecogan_pytorch_amd.ops as ops_
    from tecogan_pytorch_amd.models.networks import FRNet
    from tests.test_hip_placement import launch
    lib = L.lib()
    deg, s = 'BD', 4
    sd = generator_state_dict(scale=s, degradation=deg)
    net = FRNet(3, 3, 64, 10, deg, s)
    net.load_state_dict(sd, strict=True)
    net = net.cuda().eval()
    clip = torch.as_tensor(smooth_clip(2, 3, h, w, seed=3)).float()
    hp = torch.from_numpy(np.random.RandomState(7).uniform(0, 1, (1, 3, s * h, s * w)).astype(np.float32))
    data = (clip[1:2].contiguous(), clip[0:1].contiguous(), hp)
    plan = net._get_plan(1, h, w, torch.device('cuda', 0))
    names = [lib.tg_frnet_kind_name(k).decode() for k in range(lib.tg_frnet_plan_kinds())]
    nres = ctypes.c_int()
    L.check(lib.tg_frnet_plan_kind_stats(plan.handle, names.index('conv3x3_wino_resident_kernel'), ctypes.byref(nres), None,
                                         None), 'tg_frnet_plan_kind_stats')
    if body == 'resident' and lib.tg_conv3x3_wino_resident_supported(1, 64, h, w):
        assert nres.value == 1, 'the plan does not run the resident launch'
    elif body == 'default':
        assert nres.value == 0
    case = frnet_step_case(h, w, plan.handle, data, torch.cuda.current_stream().cuda_stream)
    ref = O.frnet_step(sd, data[0], data[1], hp, s, deg).double()
    base, launched, worst = None, [], 0.0
    for tag, pl in [('P0', {})] + case.placements():
        rc, arena, views, info = launch(lib, case, pl)
        assert rc == 0, (tag, rc, lib.tg_last_error_string())
        arena.check()
        arena.finite(views['hr_out'])
        hr = views['hr_out'].detach().cpu().contiguous()
        u8 = views['u8_out'].view(torch.uint8).cpu()
        want_u8 = ops_.quantize_u8_hwc(views['hr_out'][0]).reshape(-1).cpu()
        assert torch.equal(u8, want_u8), f'[{tag}] u8_out differs from tg_quantize_u8_hwc(hr_out) in {int((u8 != want_u8).sum())} bytes'
        assert plan.chain_state()[0] == 0, (tag, plan.chain_state())
        if base is None:
            worst = (hr.double() - ref).abs().max().item()
            assert worst <= 1e-4, worst
            base = (hr, u8)
        else:
            assert torch.equal(ints(hr), ints(base[0])), f'[{tag}] hr_out differs from the P0 result in {int((hr != base[0]).sum())} elements'
            assert torch.equal(u8, base[1]), f'[{tag}] u8_out differs from the P0 result'
        launched.append(tag)
    print(f'PLACEMENT {case.id} body={body} (resident launches per frame: {nres.value}): launched {len(launched)} '
          f'({" ".join(launched)}); refused 0 (); bit-identical to P0 in {len(launched) - 1}; worst hr_out {worst:.3e} / 1.0e-04')


@pytest.mark.parametrize('h,w,body', FRNET_STEP_CASES)
def test_frnet_step_placements(h, w, body):
    if body == 'default':
        return frnet_step_run(h, w, body)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = ('import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n'
              'from tests.test_hip_placement_chain import frnet_step_run\n'
              'frnet_step_run(%d, %d, %r)\n' % (root, os.path.join(root, 'tests', 'golden'), h, w, body))
    env = dict(os.environ, TG_WINO_RES='1', TG_CONV_WINO='1')
    r = subprocess.run([sys.executable, '-c', script], env=env, timeout=300, capture_output=True, text=True)
    print(r.stdout, end='')
    assert r.returncode == 0, r.stderr[-4000:]
