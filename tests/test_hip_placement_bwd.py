"""The gradient kernels at every buffer placement their C ABI admits (KERNELS.md, "Buffer placement", backward rows).

The method is that of tests/test_hip_placement.py, unchanged: all operands of a launch live in one Arena whose every
other word is a recognisable quiet NaN, the entry points are called through the C ABI with data_ptr() and explicit
strides, n = 2 images per segment, and every movable operand goes alone to each placement that applies to it, then all
of them together.  What the backward ABI adds:

  * segment lists (p_list, q_list, x_list, dz_list, dz_bases, act_bases, src_host): every segment is an operand of its
    own, so "segment 1 of 3 alone at P1" is a case -- the launch with ONE misaligned segment, which must drop to the
    element-wise staging as a whole.  The batch stride is shared by the segments of a list: P3 / P4 move a whole list
    (Operand.group);
  * workspaces are 'scratch' operands of EXACTLY the floats the entry's query returns for the call: Arena.check() then
    proves that nothing was written behind them.  They move to P1 / P2 where the launcher does not demand alignment;
  * a weight gradient with cb_off is the full (ca, cb_total, 3, 3) matrix, placed with finite values (Arena.inout): with
    accumulate = 0 the columns outside [cb_off, cb_off + cb) must come back bit for bit, the columns inside start as
    the guard pattern, so that finite() tells an entry that was never written;
  * the layered launch places its (1 + L, n, c, h, w) blocks with layer_stride = packed, packed + 1 (not a multiple of
    4: element-wise staging) and packed + 8 -- P0, P3 and P4 of an operand whose "images" are the layers.

Every launched placement asserts Arena.check(), Arena.finite() on every destination, the fp64 reference at the
tolerance of the entry's existing test relative to the reference's own scale (2e-5 weight gradient, 1e-5 bias
gradient, 2e-5 conv4x4s2, 1e-5 phased forward, the warps' own figures; torch.equal for what only moves data), and
bit-identity with the P0 result of the same case.  The staging forms of the weight-gradient kernels differ only in how
the values reach LDS -- same K order of the MFMAs / FMAs, same fixed-order reduce -- so every weight gradient is
identical across placements.  The two exceptions are named where they are made: BIAS_ORDER (a bias gradient whose
summation order follows the alignment of dZ) and WARP_ATOMICS.  Where a launcher refuses a placement the test asserts
the code and that nothing was written.

tests/test_placement_bwd_cpu.py restates the launchers' host-side choices and asserts that the case tables below,
crossed with the placements, reach every value of each."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_hip_placement import (Operand, Case, N, TG_E_ARG, TG_E_SHAPE, CONV4_CASES, rs, al, run_case,   # noqa: F401
                                       ops, lib)

pytestmark = pytest.mark.gpu

# ======================================================================================================================
# the case tables (plain data; the smallest shapes that still reach each form)
# ======================================================================================================================
# tg_wgrad3x3 / _multi / _multi_bias: ca, cb, cb_total, cb_off, h, w
WGRAD_CASES = [
    (64, 64, 64, 0, 3, 40),      # 2 x 32 tile, two tiles in x, vector staging at P0
    (64, 64, 64, 0, 3, 37),      # the same shape, element-wise by shape
    (64, 64, 64, 0, 6, 16),      # the 4 x 16 fold
    (64, 64, 64, 0, 6, 8),       # the 8 x 8 fold
    (32, 64, 64, 0, 3, 40),      # kmode 1: the wave pairs of the a side share a tile's pixels
    (64, 32, 32, 0, 3, 40),      # kmode 2
    (32, 32, 32, 0, 3, 40),      # kmode 3: four partials per split
    (96, 80, 80, 0, 3, 40),      # channel tails, 2 x 2 channel blocks
    (64, 48, 51, 3, 6, 8),       # conv_in's column slice: columns 0..2 belong to the other source
    (3, 64, 64, 0, 6, 8),        # small-ca (conv_out)
    (2, 40, 40, 0, 4, 72),       # small-ca (the flow head), three tiles in x
    (64, 3, 3, 0, 6, 8),         # <= 4 shifted channels: the small-ca kernel with the operands exchanged
    (64, 3, 51, 0, 6, 8),        # ... into a column slice
]
WGRAD_ENTRIES = [('single', 1), ('multi', 3), ('bias', 1)]      # tg_wgrad3x3 | tg_wgrad3x3_multi | tg_wgrad3x3_multi_bias
WGRAD_EXTRA = [('multi', 1, 0), ('bias', 3, 0), ('bias', 3, 9), ('bias', 3, 11)]      # (entry, nseg, row of WGRAD_CASES)
# tg_wgrad3x3_multi_phased: ca, cb, cphase, h, w, taps of phase coordinate 0, 1 (models/train_graph.py: the 4x4/s2
# conv passes (TAPS_12, TAPS_01), the transposed conv's gradient (TAPS_1, TAPS_01)), segments
TAPS_ALL, TAPS_01, TAPS_12, TAPS_1 = 0, 1, 2, 3
PHASED_CASES = [(64, 256, 64, 4, 8, TAPS_12, TAPS_01, 1), (64, 256, 64, 3, 40, TAPS_1, TAPS_01, 1),
                (64, 256, 64, 4, 8, TAPS_1, TAPS_01, 3)]
# tg_wgrad3x3_convt_multi: ci, co, h, w (x is (n, ci, h, w), dZ (n, co, 2h, 2w)); each with and without bias_grad
CONVT_W_CASES = [(64, 64, 3, 4), (24, 40, 3, 36), (64, 16, 2, 8), (64, 96, 2, 8)]     # the last: two co blocks, fuse_b off
CONVT_W_SEGS = (1, 2)
# tg_wgrad3x3_body / _body_bias / tg_bias_grad_body: c, layers, frames, h, w
BODY_CASES = [(64, 3, 2, 4, 8), (64, 3, 2, 5, 7)]
# tg_bias_grad / tg_bias_grad_multi: c, h, w (hw = 48 and 35), segments
BIAS_CASES = [(5, 6, 8, 1), (5, 5, 7, 1), (5, 6, 8, 3), (5, 5, 7, 3)]
# tg_conv4x4s2_dgrad: CONV4_CASES of the forward file (ci, co, h, w of the conv's INPUT) x act (0 none, 1 relu, 2 lrelu)
CONV4_ACTS = (0, 1, 2)
# tg_conv3x3_fwd_phased / _masked / _splitk: cin, cout, cphase, h, w, tapsel, taps 0, taps 1, mask, ksplit
PHASED_FWD_CASES = [
    (256, 64, 64, 4, 8, 1, TAPS_12, TAPS_01, False, 1),      # the 4x4/s2 conv's forward on s2d(x)
    (256, 64, 64, 3, 37, 1, TAPS_1, TAPS_01, True, 1),       # the transposed conv's data gradient, ReLU mask
    (64, 256, 64, 4, 8, 2, TAPS_01, TAPS_12, False, 1),      # the 4x4/s2 conv's data gradient: output phases
    (64, 256, 64, 3, 37, 2, TAPS_01, TAPS_12, True, 1),
    (256, 64, 64, 4, 8, 1, TAPS_12, TAPS_01, False, 2),      # split-K
]
# tg_depth_to_space / _act_bwd: c, h, w, s (of the INPUT (n, s s c, h, w))
D2S_CASES = [(3, 2, 4, 4), (3, 4, 4, 2), (3, 3, 5, 2), (5, 3, 4, 3)]
# tg_act_bwd / tg_maxpool2_bwd / tg_upsample_bwd: c, h, w; tg_act_bwd also on flat lengths
POINT_CASES = [(3, 6, 8), (3, 5, 7)]
ACT_FLAT = (35, 4100)
# tg_backward_warp_bwd / _bwd_acc / tg_backward_warp_s2d_bwd: c, h, w
WARP_BWD_CASES = [(3, 6, 8), (3, 5, 7), (3, 8, 72)]
WARP_MODES = ('bwd', 'acc', 's2d2', 's2d2_acc', 's2d4', 's2d4_acc')      # s2d: scale 2 / 4 where the map divides
# the data movers of tg_assemble.hip: inner (floats per frame)
MOVER_INNER = (48, 35)                   # (tg_d_assemble_*: the maps 6 x 8 and 5 x 7)


# ======================================================================================================================
# one launch at one placement
# ======================================================================================================================
class Op(Operand):
    """Operand plus: group (operands whose batch stride is ONE argument of the ABI move to P3 / P4 together), and kind
    'inout' (a destination that holds values: writable = the elements the launch may write, prefill = they start as
    the guard pattern)."""

    def __init__(self, name, kind, data=None, shape=None, strided=False, group=None, writable=None, prefill=False, **kw):
        self.inout = kind == 'inout'
        super().__init__(name, 'out' if self.inout else kind, data=data, shape=shape, strided=strided, **kw)
        self.group, self.writable, self.prefill = group, writable, prefill


class BCase(Case):
    def placements(self):
        """Base offsets (P1, P2): every operand alone.  Strides (P3, P4): an operand alone, or its whole group.  Then
        all movable operands together."""
        mov = [o for o in self.operands if o.kind != 'fixed']
        out, groups = [], {}
        for o in mov:
            for p in ('P1', 'P2'):
                out.append((f'{o.name}@{p}', {o.name: p}))
            if o.strided and o.group:
                groups.setdefault(o.group, []).append(o)
            elif o.strided:
                out += [(f'{o.name}@{p}', {o.name: p}) for p in ('P3', 'P4')]
        for g, members in groups.items():
            out += [(f'{g}@{p}', {o.name: p for o in members}) for p in ('P3', 'P4')]
        for p in ('P1', 'P2', 'P3', 'P4'):
            pl = {o.name: p for o in mov if o.resolve(p) is not None}
            if len(pl) > 1:
                out.append((f'all@{p}', pl))
        return out

    def infos(self):
        """[(tag, {operand name: (offset, stride)})] of P0 and every placement: what the CPU file crosses the
        restated launcher rules with."""
        return [(tag, {o.name: o.resolve(pl.get(o.name, 'P0')) for o in self.operands})
                for tag, pl in [('P0', {})] + self.placements()]


def rel(name, ref, tol):
    """verify(): max |got - ref| of output `name` relative to the reference's own scale (relerr of
    tests/test_hip_train_ops.py), with the bound `tol`."""
    scale = ref.abs().max().item() + 1e-30

    def verify(outs):
        got = outs[name].double()
        assert got.shape == ref.shape, (got.shape, ref.shape)
        return [(name, (got - ref).abs().max().item() / scale, tol)]
    return verify


def both(*verifiers):
    return lambda outs: [r for v in verifiers for r in v(outs)]


def exact(name, ref):
    def verify(outs):
        assert outs[name].shape == ref.shape, (outs[name].shape, ref.shape)
        return [(f'{name} (elements that differ)', float((outs[name] != ref).sum()), 0.0)]
    return verify


def ptrs(p, names):
    return (ctypes.c_void_p * len(names))(*[p[k] for k in names])


def bias_planes_as_p0(info, names, hw):
    """bias_grad_kernel / bias_grad_body_kernel read the planes of the dZ operands `names` the way they do at P0: element
    by element whatever the placement where hw % 4 != 0, else 16 bytes at a time while every plane is 16-byte aligned."""
    return hw % 4 != 0 or all_al4(info, names)


def all_al4(info, names):
    """Every operand of `names` 16-byte aligned with a stride that keeps every image so."""
    return all(al(info, k, 4) for k in names)


# ======================================================================================================================
# tg_wgrad_mfma.hip
# ======================================================================================================================
def wgrad_ref(ps, qs, stride2=False):
    """fp64: G[a][b][ky][kx] = sum P[n][a][y][x] Q[n][b][y + ky - 1][x + kx - 1] (stride2: Q at [2y - 1 + ky][2x - 1 + kx])."""
    P, Q = torch.cat(ps).double(), torch.cat(qs).double()
    h, w = P.shape[2:]
    Qp = F.pad(Q, (1, 1, 1, 1))
    G = torch.zeros(P.shape[1], Q.shape[1], 3, 3, dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            q = Qp[:, :, ky:ky + 2 * h:2, kx:kx + 2 * w:2] if stride2 else Qp[:, :, ky:ky + h, kx:kx + w]
            G[:, :, ky, kx] = torch.einsum('nayx,nbyx->ab', P, q)
    return G


def tap_on(code, k):
    return code == TAPS_ALL or (code == TAPS_01 and k <= 1) or (code == TAPS_12 and k >= 1) or (code == TAPS_1 and k == 1)


def phase_mask(channels, cphase, t0, t1):
    """(channels, 3, 3) of 0 / 1: the taps the sub-pixel phase of a channel owns (phase = channel / cphase; its row
    coordinate (phase >> 1) & 1 and column coordinate phase & 1 pick the tap set)."""
    m = torch.zeros(channels, 3, 3, dtype=torch.float64)
    sets = (t0, t1)
    for c in range(channels):
        ph = c // cphase
        for ky in range(3):
            for kx in range(3):
                m[c, ky, kx] = float(tap_on(sets[(ph >> 1) & 1], ky) and tap_on(sets[ph & 1], kx))
    return m


def wgrad_case(lib, entry, nseg, ca, cb, cb_total, cb_off, h, w, phased=None):
    """entry: 'single' tg_wgrad3x3 | 'multi' | 'bias' tg_wgrad3x3_multi_bias | 'phased' (phased = (cphase, t0, t1)).
    Every placement is accepted except, with a bias gradient, a p stride other than the packed one (TG_E_ARG: the
    stand-alone bias reduction the element-wise forms run takes no stride).

    BIAS_ORDER -- the bias gradient sums dZ in an order that follows dZ's alignment: out of the staged values of the
    vector form of the MFMA kernels (fuse_a), else by tg_bias_grad_multi, which itself reads a plane 16 bytes at a time
    only where hw % 4 == 0 and the plane is 16-byte aligned (bias_planes_as_p0).  A placement that turns fuse_a off,
    or that changes how tg_bias_grad_multi reads a plane, agrees with the P0 result to 1e-5, the bound of
    test_bias_gradient_rides_on_the_weight_gradient_launch; every other placement is bit-identical in db as well, and
    the weight gradient is bit-identical everywhere."""
    ps = [rs(10 + i, (N, ca, h, w)) for i in range(nseg)]
    qs = [rs(40 + i, (N, cb, h, w)) for i in range(nseg)]
    ref = wgrad_ref(ps, qs)
    if phased:
        ref = ref * phase_mask(cb, *phased).unsqueeze(0)
    pn, qn = [f'p{i}' for i in range(nseg)], [f'q{i}' for i in range(nseg)]
    g0 = rs(7, (ca, cb_total, 3, 3), 1.0, 2.0)
    cols = torch.zeros(1, cb_total, 1, 1, dtype=torch.bool)
    cols[:, cb_off:cb_off + cb] = True
    wsf = lib.tg_wgrad3x3_workspace_floats(N * nseg, ca, cb_total, h, w)
    opers = [Op(k, 'in', t, strided=True, group='p_list') for k, t in zip(pn, ps)] + \
            [Op(k, 'in', t, strided=True, group='q_list') for k, t in zip(qn, qs)] + \
            [Op('grad', 'inout', g0, writable=cols, prefill=True), Op('workspace', 'scratch', shape=(wsf,))]
    if entry == 'bias':
        opers.append(Op('db', 'inout', torch.full((ca,), 7.0), prefill=True))

    def call(lib, p, s):
        sp, sq = s[pn[0]], s[qn[0]]
        if entry == 'single':
            return lib.tg_wgrad3x3(p['p0'], sp, p['q0'], sq, p['grad'], p['workspace'], N, ca, cb, cb_total, cb_off, h, w, 0, None)
        a = (ptrs(p, pn), ptrs(p, qn), nseg, sp, sq, p['grad'])
        if entry == 'multi':
            return lib.tg_wgrad3x3_multi(*a, p['workspace'], N, ca, cb, cb_total, cb_off, h, w, 0, None)
        if entry == 'bias':
            return lib.tg_wgrad3x3_multi_bias(*a, p['db'], p['workspace'], N, ca, cb, cb_total, cb_off, h, w, 0, None)
        return lib.tg_wgrad3x3_multi_phased(*a, p['workspace'], N, ca, cb, h, w, 0, phased[0], phased[1], phased[2], None)

    full = g0.double().clone()
    full[:, cb_off:cb_off + cb] = ref

    def verify(outs):
        got = outs['grad'].double()
        res = [('grad', (got[:, cb_off:cb_off + cb] - ref).abs().max().item() / (ref.abs().max().item() + 1e-30), 2e-5),
               ('grad (foreign columns that changed)', float((outs['grad'][:, ~cols.view(-1)] != g0[:, ~cols.view(-1)]).sum()), 0.0)]
        if entry == 'bias':
            dbr = torch.cat(ps).double().sum((0, 2, 3))
            res.append(('db', (outs['db'].double() - dbr).abs().max().item() / dbr.abs().max().item(), 1e-5))
        return res
    def db_same(info):
        fused0 = ca > 4 and cb > 4 and w % 4 == 0                  # fuse_a at P0: an MFMA form with the vector staging
        fused = fused0 and all_al4(info, pn + qn)
        return fused0 == fused and (fused or bias_planes_as_p0(info, pn, h * w))
    return BCase(f'wgrad3x3[{entry} x{nseg}] {ca}x{cb} of {cb_total}+{cb_off} {h}x{w} {phased or ""}', opers, call, verify,
                 expect=lambda info: TG_E_ARG if entry == 'bias' and info['p0'][1] != ca * h * w else 0,
                 same_bits=lambda info: True if entry != 'bias' or db_same(info) else {'db': 1e-5})               # BIAS_ORDER


@pytest.mark.parametrize('entry,nseg', WGRAD_ENTRIES)
@pytest.mark.parametrize('ca,cb,cb_total,cb_off,h,w', WGRAD_CASES)
def test_wgrad3x3_placements(lib, entry, nseg, ca, cb, cb_total, cb_off, h, w):
    run_case(lib, wgrad_case(lib, entry, nseg, ca, cb, cb_total, cb_off, h, w))


@pytest.mark.parametrize('entry,nseg,row', WGRAD_EXTRA)
def test_wgrad3x3_placements_other_segment_counts(lib, entry, nseg, row):
    run_case(lib, wgrad_case(lib, entry, nseg, *WGRAD_CASES[row]))


@pytest.mark.parametrize('ca,cb,cphase,h,w,t0,t1,nseg', PHASED_CASES)
def test_wgrad3x3_phased_placements(lib, ca, cb, cphase, h, w, t0, t1, nseg):
    """tg_wgrad3x3_multi_phased: the 2 x 32 kernel whatever the map, the taps a phase does not own written as 0."""
    run_case(lib, wgrad_case(lib, 'phased', nseg, ca, cb, cb, 0, h, w, phased=(cphase, t0, t1)))


def convt_wgrad_case(lib, nseg, ci, co, h, w, bias):
    """tg_wgrad3x3_convt_multi takes no strides (packed segments): base offsets only.  The vector form reads x 16 and
    dZ 8 bytes at a time; one misaligned segment drops the launch to the element-wise form.  BIAS_ORDER: db rides on
    the staged dZ only in the vector form with one co block (fuse_b), else tg_bias_grad_multi runs behind the launch."""
    xs = [rs(10 + i, (N, ci, h, w)) for i in range(nseg)]
    dzs = [rs(40 + i, (N, co, 2 * h, 2 * w)) for i in range(nseg)]
    ref = wgrad_ref(xs, dzs, stride2=True)
    xn, dn = [f'x{i}' for i in range(nseg)], [f'dz{i}' for i in range(nseg)]
    wsf = lib.tg_wgrad3x3_convt_workspace_floats(N * nseg, ci, co, h, w)
    opers = [Op(k, 'in', t) for k, t in zip(xn, xs)] + [Op(k, 'in', t) for k, t in zip(dn, dzs)] + \
            [Op('grad', 'inout', rs(7, (ci, co, 3, 3), 1.0, 2.0), prefill=True), Op('workspace', 'scratch', shape=(wsf,))]
    if bias:
        opers.append(Op('db', 'inout', torch.full((co,), 7.0), prefill=True))

    def call(lib, p, s):
        return lib.tg_wgrad3x3_convt_multi(ptrs(p, xn), ptrs(p, dn), nseg, p['grad'], p.get('db'), p['workspace'], N, ci, co,
                                           h, w, 0, None)
    verify = rel('grad', ref, 2e-5)
    if bias:
        verify = both(verify, rel('db', torch.cat(dzs).double().sum((0, 2, 3)), 1e-5))
    def db_same(info):
        fused0 = w % 4 == 0 and co <= 64                           # fuse_b at P0
        fused = fused0 and all_al4(info, xn + dn)
        return fused0 == fused and (fused or bias_planes_as_p0(info, dn, 4 * h * w))
    return BCase(f'wgrad3x3_convt_multi x{nseg} {ci}->{co} {h}x{w} bias={bias}', opers, call, verify,
                 same_bits=lambda info: True if not bias or db_same(info) else {'db': 1e-5})                      # BIAS_ORDER


@pytest.mark.parametrize('bias', [False, True])
@pytest.mark.parametrize('nseg', CONVT_W_SEGS)
@pytest.mark.parametrize('ci,co,h,w', CONVT_W_CASES)
def test_wgrad3x3_convt_placements(lib, ci, co, h, w, nseg, bias):
    run_case(lib, convt_wgrad_case(lib, nseg, ci, co, h, w, bias))


def body_case(lib, entry, c, nl, frames, h, w):
    """entry 'body' tg_wgrad3x3_body | 'body_bias' | 'bias_body' tg_bias_grad_body.  The blocks are (1 + nl, n, c, h, w);
    their "images" are the layers, layer_stride floats apart: P3 (packed + 1) is the element-wise form by lstride, P4
    (packed + 8) keeps the vector form and leaves a gap behind every layer.  The nl gradients (and bias gradients) are
    one operand each, the pointers of the list point into it.  BIAS_ORDER as above: the layered launch sums dZ out
    of the staged values in the vector form, tg_bias_grad_multi layer by layer otherwise."""
    dz = [rs(50 + f, (1 + nl, N, c, h, w)) for f in range(frames)]
    act = [rs(10 + f, (1 + nl, N, c, h, w)) for f in range(frames)]
    dn, an = [f'dz{f}' for f in range(frames)], [f'act{f}' for f in range(frames)]
    wsf = lib.tg_wgrad3x3_body_workspace_floats(frames, N, nl, c, h, w)
    opers = [Op(k, 'in', t, strided=True, group='blocks') for k, t in zip(dn, dz)]
    if entry != 'bias_body':
        opers += [Op(k, 'in', t, strided=True, group='blocks') for k, t in zip(an, act)]
        opers += [Op('grads', 'inout', rs(7, (nl, c * c * 9), 1.0, 2.0), prefill=True), Op('workspace', 'scratch', shape=(wsf,))]
        gref = torch.stack([wgrad_ref([d[L] for d in dz], [a[L - 1] for a in act]).reshape(-1) for L in range(1, nl + 1)])
    nb = nl + 1 if entry == 'bias_body' else nl            # tg_bias_grad_body also does layer 0, and ADDS
    if entry != 'body':
        opers.append(Op('dbs', 'inout', torch.full((nb, c), 7.0), prefill=entry == 'body_bias'))
        layers = range(nl + 1) if entry == 'bias_body' else range(1, nl + 1)
        bref = torch.stack([torch.cat([d[L] for d in dz]).double().sum((0, 2, 3)) for L in layers]) + (7.0 if entry == 'bias_body' else 0.0)

    def call(lib, p, s):
        ls = s[dn[0]]
        if entry == 'bias_body':
            return lib.tg_bias_grad_body(ptrs(p, dn), frames, ls, nl + 1, (ctypes.c_void_p * nb)(*[p['dbs'] + 4 * c * i for i in range(nb)]),
                                         N, c, h * w, None)
        grads = (ctypes.c_void_p * nl)(*[p['grads'] + 4 * c * c * 9 * i for i in range(nl)])
        if entry == 'body':
            return lib.tg_wgrad3x3_body(ptrs(p, dn), ptrs(p, an), frames, ls, nl, grads, p['workspace'], N, c, h, w, 0, None)
        dbs = (ctypes.c_void_p * nl)(*[p['dbs'] + 4 * c * i for i in range(nl)])
        return lib.tg_wgrad3x3_body_bias(ptrs(p, dn), ptrs(p, an), frames, ls, nl, grads, dbs, p['workspace'], N, c, h, w, 0, None)
    verify = both(*([rel('grads', gref, 2e-5)] if entry != 'bias_body' else []), *([rel('dbs', bref, 1e-5)] if entry != 'body' else []))
    def db_same(info):
        fused0 = entry == 'body_bias' and w % 4 == 0               # the layered launch stages dZ 16 bytes at a time at P0
        fused = fused0 and all_al4(info, dn + an)                  # (an operand's stride is layer_stride here)
        return fused0 == fused and (fused or bias_planes_as_p0(info, dn, h * w))
    return BCase(f'{entry} c={c} layers={nl} frames={frames} {h}x{w}', opers, call, verify,
                 same_bits=lambda info: True if entry == 'body' or db_same(info) else {'dbs': 1e-5})              # BIAS_ORDER


@pytest.mark.parametrize('entry', ['body', 'body_bias', 'bias_body'])
@pytest.mark.parametrize('c,nl,frames,h,w', BODY_CASES)
def test_wgrad3x3_body_placements(lib, c, nl, frames, h, w, entry):
    run_case(lib, body_case(lib, entry, c, nl, frames, h, w))


@pytest.mark.parametrize('c,h,w,nseg', BIAS_CASES)
def test_bias_grad_placements(lib, c, h, w, nseg):
    """tg_bias_grad (one segment) / tg_bias_grad_multi, packed segments, accumulate = 1 onto 7.0: a plane is read 16
    bytes at a time where hw % 4 == 0 and the plane is 16-byte aligned, element by element otherwise (BIAS_ORDER)."""
    dys = [rs(20 + i, (N, c, h, w)) for i in range(nseg)]
    names = [f'dy{i}' for i in range(nseg)]
    ref = torch.cat(dys).double().sum((0, 2, 3)) + 7.0
    opers = [Op(k, 'in', t) for k, t in zip(names, dys)] + [Op('db', 'inout', torch.full((c,), 7.0))]

    def call(lib, p, s):
        if nseg == 1:
            return lib.tg_bias_grad(p['dy0'], p['db'], N, c, h * w, 1, None)
        return lib.tg_bias_grad_multi(ptrs(p, names), nseg, p['db'], N, c, h * w, 1, None)
    run_case(lib, BCase(f'bias_grad x{nseg} c={c} hw={h * w}', opers, call, rel('db', ref, 1e-5),
                        same_bits=lambda info: True if bias_planes_as_p0(info, names, h * w) else {'db': 1e-5}))  # BIAS_ORDER


# ======================================================================================================================
# tg_conv4x4s2_mfma.hip: the data gradient
# ======================================================================================================================
@pytest.mark.parametrize('act', CONV4_ACTS)
@pytest.mark.parametrize('ci,co,h,w', CONV4_CASES)
def test_conv4x4s2_dgrad_placements(ops, lib, ci, co, h, w, act):
    """tg_conv4x4s2_dgrad (g (n, co, h/2, w/2) -> dx (n, ci, h, w), optionally times act'(act_y)); no strides.  g is
    read element by element.  Every form stores dx -- and reads act_y -- as pairs of neighbouring pixels: 8-byte
    aligned or TG_E_ARG (the launcher let any pointer through).  The small-map forms (w = 32, 16) that split co or
    apply act'(.) run a second, 16-byte pass over dx, the workspace and act_y: 16-byte aligned or TG_E_ARG."""
    gen = torch.Generator().manual_seed(11)
    wt = torch.randn(co, ci, 4, 4, generator=gen) * 0.05
    g = torch.randn(N, co, h // 2, w // 2, generator=gen)
    act_y = torch.randn(N, ci, h, w, generator=gen)
    ref = F.conv_transpose2d(g.double(), wt.double(), None, 2, 1)
    bound = 2e-5 * ref.abs().max().item()
    if act:
        ref = torch.where(act_y.double() > 0, ref, ref * (0.2 if act == 2 else 0.0))
    _, pd = ops.pack_conv4x4s2(wt.cuda())
    wsf = lib.tg_conv4x4s2_workspace_floats(N, ci, co, h, w, 1)
    opers = [Op('g', 'in', g), Op('w', 'fixed', pd.cpu())] + ([Op('act_y', 'in', act_y)] if act else []) + \
        [Op('dx', 'out', shape=(N, ci, h, w))] + ([Op('workspace', 'scratch', shape=(wsf,))] if wsf else [])

    def call(lib, p, s):
        return lib.tg_conv4x4s2_dgrad(p['g'], p['w'], p.get('act_y'), act, p['dx'], p.get('workspace'), N, ci, co, h, w, None)

    def expect(info):
        k = 4 if w % 64 != 0 and (wsf or act) else 2
        names = ['dx'] + (['act_y'] if act else []) + (['workspace'] if wsf else [])
        return 0 if all(info[n_][0] % k == 0 for n_ in names) else TG_E_ARG

    def verify(outs):
        return [('dx', (outs['dx'].double() - ref).abs().max().item(), bound)]
    run_case(lib, BCase(f'conv4x4s2_dgrad {co}->{ci} {h}x{w} act={act} split={bool(wsf)}', opers, call, verify, expect=expect))


# ======================================================================================================================
# the phased embeddings' forward (tg_conv3x3_mfma.hip: conv3x3_mfma_kernel with phase-restricted taps)
# ======================================================================================================================
@pytest.mark.parametrize('cin,cout,cphase,h,w,tapsel,t0,t1,mask,ks', PHASED_FWD_CASES)
def test_conv3x3_fwd_phased_placements(ops, lib, cin, cout, cphase, h, w, tapsel, t0, t1, mask, ks):
    """tg_conv3x3_fwd_phased / _phased_masked / _phased_splitk reach conv3x3_impl: its batch-stride checks and its
    epilogue rule (float4 where w % 4 == 0 and y / mask are 16-byte aligned with strides % 4 == 0, per element
    otherwise; same order).  The reference is the conv with the taps a phase does not own set to zero.  The split-K
    form writes y and the partial sums packed, element by element."""
    x = rs(1, (N, cin, h, w))
    wt = rs(2, (cout, cin, 3, 3)) / (3.0 * cin ** 0.5)
    pm = phase_mask(cin if tapsel == 1 else cout, cphase, t0, t1)
    wm = wt.double() * (pm.unsqueeze(0) if tapsel == 1 else pm.unsqueeze(1))
    m = rs(5, (N, cout, h, w)) if mask else None
    ref = F.conv2d(x.double(), wm, None, padding=1)
    if mask:
        ref = torch.where(m.double() > 0, ref, torch.zeros_like(ref))
    pk, _, _, ocb = ops.pack_conv3x3(wt.cuda())
    opers = [Op('x', 'in', x, strided=True)] + ([Op('mask', 'in', m, strided=True)] if mask else []) + [Op('w', 'fixed', pk.cpu())]
    if ks > 1:
        opers += [Op('partials', 'scratch', shape=(ks * N * cout * h * w,)), Op('y', 'out', shape=(N, cout, h, w))]
    else:
        opers.append(Op('y', 'out', shape=(N, cout, h, w), strided=True))

    def call(lib, p, s):
        if ks > 1:
            return lib.tg_conv3x3_fwd_phased_splitk(p['x'], s['x'], p['w'], ocb, None, p['y'], N, cin, cout, h, w, 0, tapsel, cphase,
                                                    t0, t1, ks, p['partials'], None)
        if mask:
            return lib.tg_conv3x3_fwd_phased_masked(p['x'], s['x'], p['w'], ocb, None, p['mask'], s['mask'], p['y'], s['y'], N, cin,
                                                    cout, h, w, 0, tapsel, cphase, t0, t1, None)
        return lib.tg_conv3x3_fwd_phased(p['x'], s['x'], p['w'], ocb, None, p['y'], s['y'], N, cin, cout, h, w, 0, tapsel, cphase,
                                         t0, t1, None)

    def verify(outs):
        return [('y', (outs['y'].double() - ref).abs().max().item(), 1e-5)]
    run_case(lib, BCase(f'conv3x3_fwd_phased tapsel={tapsel} {cin}->{cout} {h}x{w} mask={mask} ks={ks}', opers, call, verify))


# ======================================================================================================================
# tg_train.hip: the glue kernels' gradients
# ======================================================================================================================
@pytest.mark.parametrize('act', [0, 1, 2])
@pytest.mark.parametrize('c,h,w,s', D2S_CASES)
def test_depth_to_space_placements(lib, c, h, w, s, act):
    """tg_depth_to_space (act 0; no strides): the 16-byte form where s is 2 or 4, w % 4 == 0 and x, y are 16-byte
    aligned, the element form otherwise.  tg_depth_to_space_act_bwd (relu | lrelu) has the 16-byte form only: TG_E_ARG
    unless s is 2 or 4, w % 4 == 0 and x, act_y, y are 16-byte aligned.  A permutation (times 0, 0.2 or 1): exact."""
    from oracle import tecogan_oracle as O
    y0 = rs(1, (N, c, s * h, s * w))
    x = O.space_to_depth(y0, s).contiguous()            # depth_to_space inverts it
    act_y = rs(2, (N, c, s * h, s * w))
    ref = y0 if not act else torch.where(act_y > 0, y0, y0 * (0.2 if act == 2 else 0.0))
    opers = [Op('x', 'in', x)] + ([Op('act_y', 'in', act_y)] if act else []) + [Op('y', 'out', shape=tuple(y0.shape))]

    def call(lib, p, s_):
        if act:
            return lib.tg_depth_to_space_act_bwd(p['x'], p['act_y'], act, p['y'], N, c, h, w, s, None)
        return lib.tg_depth_to_space(p['x'], p['y'], N, c, h, w, s, None)

    def expect(info):
        ok = s in (2, 4) and w % 4 == 0 and all(v[0] % 4 == 0 for v in info.values())
        return 0 if not act or ok else TG_E_ARG
    run_case(lib, BCase(f'depth_to_space c={c} {h}x{w} s={s} act={act}', opers, call, exact('y', ref), expect=expect))


def _act_bwd_case(lib, shape, act):
    z = rs(1, shape, -2, 2).double()
    y = {1: torch.relu(z), 2: torch.where(z > 0, z, 0.2 * z), 3: torch.tanh(z) * 24}[act].float()
    dy = rs(2, shape)
    ref = dy.double() * {1: (y > 0).double(), 2: torch.where(y > 0, 1.0, 0.2).double(), 3: 24.0 - y.double() ** 2 / 24.0}[act]
    n = int(np.prod(shape))
    opers = [Op('dy', 'in', dy), Op('y', 'in', y), Op('dx', 'out', shape=shape)]
    run_case(lib, BCase(f'act_bwd {shape} act={act}', opers, lambda lib, p, s: lib.tg_act_bwd(p['dy'], p['y'], p['dx'], n, act, None),
                        rel('dx', ref, 2e-5 if act == 3 else 1e-7)))


@pytest.mark.parametrize('act', [1, 2, 3])
@pytest.mark.parametrize('shape', [(N,) + c for c in POINT_CASES] + [(k,) for k in ACT_FLAT])
def test_act_bwd_placements(lib, shape, act):
    """tg_act_bwd: element by element over a flat length, any base; test_act_bwd's bounds."""
    _act_bwd_case(lib, shape, act)


@pytest.mark.parametrize('c,h,w', POINT_CASES)
def test_maxpool2_bwd_placements(lib, c, h, w):
    """tg_maxpool2_bwd (no strides), element by element; the gradient goes to the first maximum of a window: exact."""
    x = rs(2, (N, c, h, w)).requires_grad_(True)
    g = rs(3, (N, c, h // 2, w // 2))
    F.max_pool2d(x, 2, 2).backward(g)
    opers = [Op('x', 'in', x.detach()), Op('dy', 'in', g), Op('dx', 'out', shape=(N, c, h, w))]
    run_case(lib, BCase(f'maxpool2_bwd c={c} {h}x{w}', opers,
                        lambda lib, p, s: lib.tg_maxpool2_bwd(p['x'], p['dy'], p['dx'], N * c, h, w, None), exact('dx', x.grad)))


@pytest.mark.parametrize('deg,s', [('BD', 4), ('BI', 2)])
@pytest.mark.parametrize('c,h,w', POINT_CASES)
def test_upsample_bwd_placements(ops, lib, c, h, w, deg, s):
    """tg_upsample_bwd, both modes (no strides): a gather, element by element; test_upsample_bwd's bound."""
    from oracle import tecogan_oracle as O
    x = rs(1, (N, c, h, w)).double().requires_grad_(True)
    g = rs(2, (N, c, h * s, w * s))
    (float(s) * O.upsample(x, s, deg)).backward(g.double())
    opers = [Op('dy', 'in', g), Op('dx', 'out', shape=(N, c, h, w))]
    run_case(lib, BCase(f'upsample_bwd {deg} x{s} c={c} {h}x{w}', opers,
                        lambda lib, p, s_: lib.tg_upsample_bwd(p['dy'], p['dx'], N * c, h, w, s, ops.UP_MODE[deg], float(s), None),
                        rel('dx', x.grad, 1e-5)))


@pytest.mark.parametrize('c,h,w,mode', [(c, h, w, m) for c, h, w in WARP_BWD_CASES for m in WARP_MODES
                                        if not m.startswith('s2d') or (h % int(m[3]) == 0 and w % int(m[3]) == 0)])
def test_backward_warp_bwd_placements(lib, c, h, w, mode):
    """tg_backward_warp_bwd / _bwd_acc / tg_backward_warp_s2d_bwd (both accumulate; scale 2 and 4 where the map
    divides): no strides, element by element, every base offset accepted.  WARP_ATOMICS -- the image gradient is
    scattered with atomic adds and is not identical run to run: both gradients are held to the figures of
    test_backward_warp_bwd only (2e-5 of its scale for dimg; dflow within 1e-3 of its scale except at the < 0.2 % of
    positions that sit on a kink of the bilinear kernel)."""
    from oracle import tecogan_oracle as O
    s2d = int(mode[3]) if mode.startswith('s2d') else 1
    acc = mode.endswith('acc')
    x = rs(1, (N, c, h, w), 0, 1).double().requires_grad_(True)
    fl = (rs(2, (N, 2, h, w)) * 3.0).double().requires_grad_(True)
    g = rs(3, (N, c, h, w))
    O.backward_warp(x, fl).backward(g.double())
    dy = O.space_to_depth(g, s2d).contiguous() if s2d > 1 else g
    prior = rs(4, (N, c, h, w))
    dimg_ref = x.grad + (prior.double() if acc else 0.0)
    opers = [Op('x', 'in', x.detach().float()), Op('flow', 'in', fl.detach().float()), Op('dy', 'in', dy),
             Op('dimg', 'inout', prior) if acc else Op('dimg', 'out', shape=(N, c, h, w)), Op('dflow', 'out', shape=(N, 2, h, w))]

    def call(lib, p, s):
        if s2d > 1:
            return lib.tg_backward_warp_s2d_bwd(p['x'], p['flow'], p['dy'], p['dimg'], 1 if acc else 0, p['dflow'], N, c, h, w, s2d, None)
        if acc:
            return lib.tg_backward_warp_bwd_acc(p['x'], p['flow'], p['dy'], p['dimg'], p['dflow'], N, c, h, w, None)
        return lib.tg_backward_warp_bwd(p['x'], p['flow'], p['dy'], p['dimg'], p['dflow'], N, c, h, w, None)

    def verify(outs):
        d = (outs['dflow'].double() - fl.grad).abs()
        return [('dimg', (outs['dimg'].double() - dimg_ref).abs().max().item() / dimg_ref.abs().max().item(), 2e-5),
                ('dflow (share off by > 1e-3 of its scale)', (d > 1e-3 * fl.grad.abs().max()).double().mean().item(), 2e-3)]
    run_case(lib, BCase(f'backward_warp_bwd[{mode}] c={c} {h}x{w}', opers, call, verify, same_bits=lambda info: False))   # WARP_ATOMICS


# ======================================================================================================================
# tg_assemble.hip: the data movers (exact)
# ======================================================================================================================
def _inner_shape(inner):
    return (3, 4, 4) if inner == 48 else (5, 7)


@pytest.mark.parametrize('inner', MOVER_INNER)
def test_time_gather_and_transpose01_placements(lib, inner):
    """tg_time_gather (x (n, t, inner) -> (n, k, inner), idx < 0: zeros) and tg_transpose01 move 16 bytes at a time:
    inner % 4 == 0 (TG_E_SHAPE / TG_E_ARG) and both pointers 16-byte aligned (TG_E_ARG); there is no element form."""
    sh = _inner_shape(inner)
    x = rs(1, (N, 5) + sh)
    idx = [3, -1, 0, 4]
    ref = torch.stack([x[:, i] if i >= 0 else torch.zeros_like(x[:, 0]) for i in idx], 1)
    cidx = (ctypes.c_int * len(idx))(*idx)
    ok = lambda info: all(v[0] % 4 == 0 for v in info.values())       # noqa: E731
    run_case(lib, BCase(f'time_gather inner={inner}', [Op('x', 'in', x), Op('y', 'out', shape=tuple(ref.shape))],
                        lambda lib, p, s: lib.tg_time_gather(p['x'], p['y'], cidx, N, 5, len(idx), inner, None), exact('y', ref),
                        expect=lambda info: TG_E_SHAPE if inner % 4 else (0 if ok(info) else TG_E_ARG)))
    xt = rs(2, (3, 5) + sh)
    run_case(lib, BCase(f'transpose01 inner={inner}', [Op('x', 'in', xt), Op('y', 'out', shape=(5, 3) + sh)],
                        lambda lib, p, s: lib.tg_transpose01(p['x'], p['y'], 3, 5, inner, None), exact('y', xt.transpose(0, 1).contiguous()),
                        expect=lambda info: 0 if inner % 4 == 0 and ok(info) else TG_E_ARG))


@pytest.mark.parametrize('inner', MOVER_INNER)
def test_stack_time_placements(lib, inner):
    """tg_stack_time (k sources (n, inner) -> y (n, k, inner)), 16 bytes at a time: every source AND y 16-byte aligned
    -- the launcher checked the sources and cast y unchecked; TG_E_ARG now, which y@P1 / y@P2 assert.  Each source is
    an operand of its own: "source 1 of 3 alone at P1" is refused as a whole."""
    sh = _inner_shape(inner)
    frames = [rs(10 + j, (N,) + sh) for j in range(3)]
    names = [f'src{j}' for j in range(3)]
    opers = [Op(k, 'in', t) for k, t in zip(names, frames)] + [Op('y', 'out', shape=(N, 3) + sh)]
    run_case(lib, BCase(f'stack_time inner={inner}', opers,
                        lambda lib, p, s: lib.tg_stack_time(ptrs(p, names), 3, p['y'], N, inner, None), exact('y', torch.stack(frames, 1)),
                        expect=lambda info: 0 if inner % 4 == 0 and all(v[0] % 4 == 0 for v in info.values()) else TG_E_ARG))


@pytest.mark.parametrize('inner', MOVER_INNER)
def test_pingpong_grad_and_index_gather_placements(lib, inner):
    """tg_pingpong_grad (g (n, te - 1, inner) -> +g | 0 | -flip(g)) and tg_index_gather (both accumulate): element by
    element, any base and any inner."""
    sh, te = _inner_shape(inner), 4
    g = rs(1, (N, te - 1) + sh)
    want = torch.zeros((N, 2 * te - 1) + sh)
    want[:, :te - 1] = g
    want[:, te:] = -g.flip(1)
    run_case(lib, BCase(f'pingpong_grad inner={inner}', [Op('g', 'in', g), Op('out', 'out', shape=tuple(want.shape))],
                        lambda lib, p, s: lib.tg_pingpong_grad(p['g'], p['out'], N, te, inner, None), exact('out', want)))
    src = rs(2, (inner,))
    idx = torch.from_numpy(np.random.RandomState(3).randint(0, inner + 2, (2 * inner + 1,)).astype(np.int64))      # inner, inner + 1: out of range -> 0
    prior = rs(4, (idx.numel(),))
    got = torch.where(idx < inner, src[idx.clamp(max=inner - 1)], torch.zeros(()))
    idx_dev = idx.cuda()                                 # (int64: kept outside the arena of 32-bit words)
    for accumulate in (0, 1):
        opers = [Op('src', 'in', src), Op('out', 'inout', prior) if accumulate else Op('out', 'out', shape=(idx.numel(),))]
        run_case(lib, BCase(f'index_gather n_src={inner} acc={accumulate}', opers,
                            lambda lib, p, s: lib.tg_index_gather(p['src'], idx_dev.data_ptr(), p['out'], idx.numel(), inner, accumulate, None),
                            exact('out', prior + got if accumulate else got)))


@pytest.mark.parametrize('t_data,pad', [(4, 1), (3, 0)])
@pytest.mark.parametrize('inner', MOVER_INNER)
def test_d_assemble_placements(lib, inner, t_data, pad):
    """tg_d_assemble_fwd / _bwd (no strides), element by element: any base, on the 6 x 8 map (inner = 48) and the odd
    5 x 7 map (inner = 35); with and without frames beyond t and a padded crop."""
    H, W = (6, 8) if inner == 48 else (5, 7)
    assert H * W == inner
    n, t, c, crop = N, 3, 3, H - 2 * pad
    data, warped, cond = rs(1, (n, t_data, c, H, W)), rs(2, (n * t, c, H, W)), rs(3, (n, t_data, c, H, W))
    d, wp = data.clone().requires_grad_(True), warped.clone().requires_grad_(True)
    nclip = n * t // 3

    def trip(v):
        return v.reshape(nclip, 3, c, H, W).permute(0, 2, 1, 3, 4).reshape(nclip, 3 * c, H, W)
    wc = F.pad(trip(wp)[:, :, pad:pad + crop, pad:pad + crop], (pad, W - pad - crop, pad, H - pad - crop))
    want = torch.cat([trip(d[:, :t].reshape(n * t, c, H, W)), wc, trip(cond[:, :t].reshape(n * t, c, H, W))], 1)
    opers = [Op('data', 'in', data), Op('warped', 'in', warped), Op('cond', 'in', cond), Op('x', 'out', shape=tuple(want.shape))]
    run_case(lib, BCase(f'd_assemble_fwd t_data={t_data} pad={pad} crop={crop}', opers,
                        lambda lib, p, s: lib.tg_d_assemble_fwd(p['data'], t_data, p['warped'], p['cond'], t_data, p['x'], n, t, c, H, W,
                                                                pad, crop, None), exact('x', want.detach())))
    gy = rs(4, tuple(want.shape))
    want.backward(gy)
    opers = [Op('g', 'in', gy), Op('g_data', 'out', shape=tuple(data.shape)), Op('g_warped', 'out', shape=tuple(warped.shape))]
    run_case(lib, BCase(f'd_assemble_bwd t_data={t_data} pad={pad} crop={crop}', opers,
                        lambda lib, p, s: lib.tg_d_assemble_bwd(p['g'], p['g_data'], t_data, p['g_warped'], n, t, c, H, W, pad, crop, None),
                        both(exact('g_data', d.grad), exact('g_warped', wp.grad))))
