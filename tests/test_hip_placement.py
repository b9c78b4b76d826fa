"""The forward kernels at every buffer placement their C ABI admits (KERNELS.md, "Buffer placement").

Every other GPU test hands each operand its own fresh, 512-byte aligned, packed allocation.  Here ALL operands of a
launch live in one allocation (tests/placement.py: Arena) whose every other word is a recognisable quiet NaN, the
entry points are called through the C ABI with data_ptr() and explicit strides (the way ops.py calls them; its
wrappers insist on contiguous tensors and compute packed strides), and each operand is moved in turn:

    P1 base + 1 float | P2 base + 2 floats | P3 nstride = packed + 1 | P4 nstride = packed + 8 |
    P5 the destination is the first cout channels of an (n, cout + 3, h, w) buffer

first one operand alone, then all of them together, always with n = 2 so that image 1 exists.  What a launcher does
with a placement was read off its code first: a placement is launched only where every access is in bounds and legally
aligned, and where the launcher refuses, the test asserts the code and that nothing was written.

Every launched placement asserts
  * Arena.check(): no guard word, no gap between images and no foreign operand changed,
  * Arena.finite(): every element of the logical output written and finite (0 * NaN is NaN: a kernel that reads
    past a tensor and relies on a zero weight fails; in production the neighbour holds anything),
  * the tolerance of the entry point's existing test against the same fp64 reference (1e-5 for the conv forms, 2e-5
    with the tanh * 24 epilogue, the fp16 file's derived bound, the glue kernels' own figures),
  * bit-identity with the P0 result: the forms a placement selects differ in store width and addressing, not in
    summation order.  The one exception is named where it is made (SMALL_KS below).

The case tables are plain data: tests/test_placement_cpu.py restates the launchers' host-side choices and asserts that
these tables reach every value of each."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tecogan_pytorch_amd._lib import TG_E_SHAPE, TG_E_ARG
from tests.placement import Arena, PLACEMENTS, extent_floats

pytestmark = pytest.mark.gpu

N = 2                            # image 1 exists in every case


def rs(seed, shape, lo=-1.0, hi=1.0):
    return torch.from_numpy(np.random.RandomState(seed).uniform(lo, hi, shape).astype(np.float32))


def act_ref(t, act):
    return {0: t, 1: torch.relu(t), 2: torch.where(t >= 0, t, t * 0.2), 3: torch.tanh(t) * 24}[act]


def act_tol(act):
    return 2e-5 if act == 3 else 1e-5


@pytest.fixture(scope='module')
def ops():
    import tecogan_pytorch_amd.ops as ops_
    return ops_


@pytest.fixture(scope='module')
def lib():
    from tecogan_pytorch_amd import _lib
    return _lib.lib()


# ======================================================================================================================
# the case tables (plain data; shapes: the smallest that still reach each form)
# ======================================================================================================================
# tg_conv3x3_fwd / tg_conv3x3_fwd_masked: cin, cout, h, w, act, c1 (two sources), residual, mask
MFMA_CASES = [
    (51, 64, 6, 8, 1, 3, True, False),       # 3 + 48 -> 64, K padded 51 -> 56: the one-shot kernel, w % 4 == 0
    (51, 64, 5, 7, 1, 3, True, False),       # ... on an odd map
    (27, 64, 6, 8, 2, None, True, True),     # K padded 27 -> 32: the 2-row tile, residual and ReLU mask
    (27, 64, 5, 7, 2, None, False, True),
    (16, 48, 3, 40, 0, None, False, False),  # cout = 48, two workgroups in x, w % 4 == 0
    (16, 48, 3, 37, 0, None, True, False),   # ... ragged second tile
    (6, 32, 6, 8, 2, 3, False, False),       # cout <= 32: ocb 32 (the 4-row, one-tile-per-wave variant), two sources
    (6, 32, 5, 7, 2, 3, True, True),
    (128, 128, 4, 8, 2, None, True, False),  # two oc groups, K split over the wave groups of a workgroup
]
# tg_conv3x3_splitk_fwd: cin, cout, h, w, c1, ksplit, pool
SPLITK_CASES = [
    (64, 64, 6, 8, None, 2, False), (64, 64, 6, 8, None, 2, True), (51, 64, 5, 7, 3, 4, True), (27, 48, 3, 40, None, 2, False),
]
# tg_conv3x3s2_fwd: cin, cout, h_out, w_out, act, mask
S2_CASES = [(64, 64, 3, 4, 0, True), (40, 48, 3, 5, 1, False), (64, 64, 2, 34, 0, True)]
# tg_conv3x3_wino_fwd: cin, cout, h, w, act, c1, residual, mask
WINO_CASES = [
    (51, 64, 6, 8, 1, 3, True, False),       # two sources, K padded 51 -> 64; 8 x 8-pixel tiles (tr 4)
    (51, 64, 5, 7, 1, 3, True, True),        # odd map: scalar stores whatever the placement
    (27, 64, 6, 8, 3, None, False, True),    # K padded 27 -> 32, tanh * 24
    (64, 48, 3, 40, 0, None, True, False),   # cout = 48, 4 x 16-pixel tiles (tr 2), three workgroups in x
    (16, 64, 2, 36, 2, None, True, True),    # 2 x 32-pixel tiles (tr 1), two workgroups in x
    (16, 64, 2, 35, 2, None, True, False),
    (32, 32, 6, 8, 2, None, True, True),     # cout <= 32: the 32-channel workgroup, tr 4
    (32, 32, 4, 24, 1, None, True, False),   # ... tr 2
    (32, 16, 2, 72, 0, None, False, True),   # ... tr 1, two workgroups in x
    (128, 128, 4, 8, 2, None, True, False),  # two oc groups
]
# tg_conv3x3_wino_fused_fwd: cin, cout, h, w (the conv's own map), act, fuse (1 POOL, 2 UP2)
WINO_FUSED_CASES = [
    (32, 32, 6, 8, 2, 1), (16, 64, 2, 36, 2, 1), (27, 48, 4, 40, 1, 1),
    (32, 32, 6, 8, 2, 2), (64, 64, 2, 36, 2, 2), (27, 48, 4, 40, 1, 2),
]
# tg_conv3x3_small_fwd: cin, cout, h, w, act, up (None | (mode, scale))
SMALL_CASES = [
    (32, 2, 6, 8, 3, None),                  # the flow head: tanh * 24; few tiles -> the channel-split 4-row form at P0
    (32, 2, 5, 7, 3, None),                  # odd map: the scalar form
    (9, 3, 3, 72, 1, None),                  # two workgroups in x
    (64, 3, 8, 8, 0, ('BD', 4)),             # conv_out with the bicubic residual: the 16-byte form at P0
    (64, 3, 6, 8, 0, ('BI', 2)),
    (64, 3, 6, 10, 0, ('BI', 2)),            # w % 4 != 0 with a residual
]
# tg_conv3x3_small_fwd_res / tg_conv3x3_fewin_fwd: cin, cout, h, w, act
SMALL_RES_CASES = [(64, 3, 6, 8, 0), (32, 2, 4, 72, 1), (64, 3, 5, 7, 0)]          # (the last: refused at P0 already)
FEWIN_CASES = [(3, 64, 6, 8, True), (2, 40, 4, 72, False), (3, 64, 5, 7, True)]    # cin, cout, h, w, mask
# tg_convt3x3s2_fwd: cin, cout, h, w
CONVT_CASES = [(64, 64, 3, 4), (51, 37, 5, 7), (16, 40, 2, 34), (72, 64, 3, 8)]    # the last: the chunk-by-chunk kernel
# tg_convt3x3s2_z_fwd_form / tg_convt3x3s2_z_wino_fwd: cin, cout, cz, h, w
CONVT_Z_CASES = [(64, 64, 3, 3, 4), (40, 48, 2, 5, 7), (64, 64, 1, 2, 34)]
Z_FORMS = (-1, 0, 3)             # every form tg_convt3x3s2_z_fwd_form still accepts
Z_WINO_SPLITS = (-1, 0, 1)
# tg_convout_tail_form: cz, h, w, up
TAIL_CASES = [(3, 6, 8, ('BD', 2)), (2, 5, 7, None), (3, 4, 72, ('BI', 2)), (1, 2, 264, None)]
TAIL_FORMS = (-1, 0, 1)
# fp16: tg_conv3x3_f16_pack_input (c1, c2, h, w), tg_conv3x3_f16_fwd (h, w, relu, skip), tg_convt3x3s2_f16_fwd (h, w, relu)
F16_PACK_CASES = [(3, 48, 5, 7), (3, 12, 6, 8), (64, 0, 3, 40)]
F16_CONV_CASES = [(5, 7, True, True), (6, 8, False, False), (3, 40, True, False)]
F16_CONVT_CASES = [(3, 4, True), (5, 7, False), (2, 40, True)]
# the glue kernels
WARP_CASES = [(3, 6, 8), (3, 5, 7), (2, 3, 72)]                                       # c, h, w
FLOWUP_CASES = [('BD', 4, 8, 8), ('BI', 2, 9, 13), ('BD', 2, 8, 12), ('BI', 4, 10, 72)]   # deg, s, h, w (LR)
S2D_CASES = [(3, 8, 16, 4), (3, 8, 8, 2), (3, 6, 10, 2), (5, 9, 12, 3)]               # c, h, w, s
UPSAMPLE_CASES = [(3, 6, 8, 2, 'BI'), (3, 5, 7, 2, 'BI'), (3, 3, 4, 4, 'BD'), (2, 5, 7, 4, 'BI')]   # c, h, w, s, deg
MAXPOOL_CASES = [(5, 6, 8), (5, 5, 7), (3, 9, 12)]                                    # c, h, w
CONV4_CASES = [(64, 64, 8, 32), (64, 128, 16, 16), (64, 64, 2, 64), (64, 64, 2, 128)]  # ci, co, h, w


# ======================================================================================================================
# one launch at one placement
# ======================================================================================================================
class Operand:
    """kind: 'in' (moved), 'fixed' (weights, bias: placed aligned, never moved), 'out', 'scratch' (a destination whose
    content is not part of the result).  strided: the ABI takes a batch stride for it.  packed: that stride at P0
    where it is not the product of the trailing dimensions (the 32 planes of a Z buffer of which 9 cz are used)."""

    def __init__(self, name, kind, data=None, shape=None, strided=False, packed=None, p5=False, dtype=torch.float32):
        self.name, self.kind, self.data, self.strided, self.p5, self.dtype = name, kind, data, strided, p5, dtype
        self.shape = tuple(data.shape) if data is not None else tuple(shape)
        if data is not None:
            self.dtype = data.dtype
        per = int(np.prod(self.shape[1:])) if len(self.shape) > 1 else self.shape[0]
        self.packed = per if packed is None else packed
        self.itemsize = torch.empty(0, dtype=self.dtype).element_size()

    def resolve(self, placement):
        """(offset in floats, batch stride in elements) under placement 'P0'..'P5', or None where it does not apply."""
        off, extra, p5 = PLACEMENTS[placement]
        if self.kind == 'fixed':
            return None if placement != 'P0' else (0, self.packed)
        if p5:
            if not (self.p5 and self.strided):
                return None
            c = self.shape[1]
            return 0, self.packed // c * (c + 3)
        if extra and not self.strided:
            return None
        return off, self.packed + extra * 4 // self.itemsize        # (+1 / +8 FLOATS for a 16-bit operand as well)


class Case:
    def __init__(self, ident, operands, call, verify, expect=None, same_bits=None):
        self.id, self.operands, self.call, self.verify = ident, operands, call, verify
        self.expect = expect or (lambda info: 0)
        self.same_bits = same_bits or (lambda info: True)

    def placements(self):
        """[(tag, {operand name: placement})]: each movable operand alone at each placement that applies to it, then
        all of them together."""
        mov = [o for o in self.operands if o.kind != 'fixed']
        out = []
        for o in mov:
            for p in ('P1', 'P2', 'P3', 'P4', 'P5'):
                if o.resolve(p) is not None:
                    out.append((f'{o.name}@{p}', {o.name: p}))
        for p in ('P1', 'P2', 'P3', 'P4'):
            pl = {o.name: p for o in mov if o.resolve(p) is not None}
            if len(pl) > 1:
                out.append((f'all@{p}', pl))
        return out


def launch(lib, case, pl):
    """Place every operand as `pl` says (default P0), call the entry point, return (rc, arena, views, info)."""
    info = {o.name: o.resolve(pl.get(o.name, 'P0')) for o in case.operands}
    ext = [extent_floats(o.shape, info[o.name][1] if len(o.shape) > 1 else None, o.itemsize) for o in case.operands]
    arena = Arena('cuda', margin_floats=max(ext) + 64, slots=len(case.operands),
                  align_floats=max(getattr(o, 'align', 16) for o in case.operands))
    views = {}
    for o in case.operands:
        off, ns = info[o.name]
        kw = dict(offset_floats=off, nstride=ns if len(o.shape) > 1 else None, name=o.name)
        if getattr(o, 'inout', False):      # (tests/test_hip_placement_bwd.py: a destination that already holds values)
            views[o.name] = arena.inout(o.data, o.writable, o.prefill, **kw)
        else:
            # (tests/test_hip_placement_chain.py: a workspace that wants its own alignment / to start as zeros)
            extra = {k: v for k, v in (('align_floats', getattr(o, 'align', None)), ('zero', getattr(o, 'zero', None))) if v}
            views[o.name] = arena.place(o.data, **kw) if o.data is not None else arena.out(o.shape, dtype=o.dtype, **kw, **extra)
    ptr = {k: v.data_ptr() for k, v in views.items()}
    ns = {k: v[1] for k, v in info.items()}
    torch.cuda.synchronize()
    rc = case.call(lib, ptr, ns)
    torch.cuda.synchronize()
    return rc, arena, views, info


def run_case(lib, case):
    """P0 first (the baseline every other placement must reproduce bit for bit), then every placement of the case.
    All placements run; the failures are reported together, each with its tag."""
    failures, launched, rejected, worst, bits_checked, bits_skipped = [], [], [], {}, 0, []
    base = None
    for tag, pl in [('P0', {})] + case.placements():
        rc, arena, views, info = launch(lib, case, pl)
        want = case.expect(info)
        try:
            if rc != want:
                msg = lib.tg_last_error_string().decode('utf-8', 'replace') if rc else ''
                raise AssertionError(f'returned {rc}, the launcher\'s code says {want} ({msg})')
            if want != 0:
                arena.check(outputs_untouched=True)        # refused: nothing may have been launched
                assert lib.tg_last_error_string(), 'a refusal carries a message'
                rejected.append(f'{tag}:{want}')
                continue
            arena.check()
            outs = {}
            for o in case.operands:
                if o.kind == 'out':
                    arena.finite(views[o.name])
                    outs[o.name] = views[o.name].detach().cpu().contiguous()
            for what, value, bound in case.verify(outs):
                k = worst.setdefault(what, [0.0, bound])
                k[0] = max(k[0], value)
                assert value <= bound, f'{what}: {value:.3e} > {bound:.3e}'
            same = base is None or case.same_bits(info)
            if base is None:
                base = outs
            elif same:
                # same: True, or {output: bound} for the outputs that agree with the P0 result only to `bound` of its
                # scale (the others bit for bit)
                loose = same if isinstance(same, dict) else {}
                for k, v in outs.items():
                    if k in loose:
                        d = (v.double() - base[k].double()).abs().max().item() / (base[k].double().abs().max().item() + 1e-30)
                        assert d <= loose[k], f'{k} is {d:.3e} of its scale from the P0 result (bound {loose[k]:.1e})'
                        continue
                    as_int = torch.int32 if v.element_size() == 4 else torch.int16
                    assert torch.equal(v.view(as_int), base[k].view(as_int)), f'{k} differs from the P0 result in {int((v != base[k]).sum())} elements, ' \
                                 f'max |d| {(v.double() - base[k].double()).abs().max().item():.3e}'
                if loose:
                    bits_skipped.append(tag)
                else:
                    bits_checked += 1
            else:
                bits_skipped.append(tag)
            launched.append(tag)
        except AssertionError as e:
            failures.append(f'[{case.id} {tag}] {e}')
    print(f'PLACEMENT {case.id}: launched {len(launched)} ({" ".join(launched)}); refused {len(rejected)} '
          f'({" ".join(rejected)}); bit-identical to P0 in {bits_checked}, fp64 bound only in {len(bits_skipped)} '
          f'({" ".join(bits_skipped)}); worst ' + ', '.join(f'{k} {v[0]:.3e} / {v[1]:.1e}' for k, v in worst.items()))
    assert not failures, '\n'.join(failures)
    assert base is not None or case.expect({o.name: o.resolve('P0') for o in case.operands}) != 0


def maxerr(name, ref, tol):
    """verify(): the maximum absolute error of output `name` against the fp64 reference, with the bound `tol`."""
    def verify(outs):
        got = outs[name].double()
        assert got.shape == ref.shape, (got.shape, ref.shape)
        return [(name, (got - ref).abs().max().item(), tol)]
    return verify


def al(info, name, k):
    """Operand `name` is aligned to k floats: base offset and batch stride (in floats) are multiples of k."""
    off, ns = info[name]
    return off % k == 0 and ns % k == 0


# ======================================================================================================================
# tg_conv3x3_mfma.hip
# ======================================================================================================================
def _conv_inputs(cin, cout, h, w, act, c1, res, mask):
    x = rs(1, (N, cin, h, w))
    wt = rs(2, (cout, cin, 3, 3)) / (3.0 * cin ** 0.5)
    b = rs(3, (cout,), -0.5, 0.5)
    r = rs(4, (N, cout, h, w)) if res else None
    m = rs(5, (N, cout, h, w)) if mask else None
    ref = act_ref(F.conv2d(x.double(), wt.double(), b.double(), padding=1), act)
    if res:
        ref = ref + r.double()
    if mask:
        ref = torch.where(m.double() > 0, ref, torch.zeros_like(ref))
    opers = [Operand('x', 'in', x[:, :c1].contiguous() if c1 else x, strided=True)]
    if c1:
        opers.append(Operand('x2', 'in', x[:, c1:].contiguous(), strided=True))
    if res:
        opers.append(Operand('res', 'in', r, strided=True))
    if mask:
        opers.append(Operand('mask', 'in', m, strided=True))
    return x, wt, b, ref, opers


@pytest.mark.parametrize('cin,cout,h,w,act,c1,res,mask', MFMA_CASES)
def test_conv3x3_mfma_placements(ops, lib, cin, cout, h, w, act, c1, res, mask):
    """tg_conv3x3_fwd (plain, two-source, residual) and tg_conv3x3_fwd_masked: the launcher accepts every placement
    (inputs through 4-byte buffer loads bounded per image; the epilogue is the float4 form only where w % 4 == 0 and
    y / res / mask are 16-byte aligned with strides % 4 == 0, else one store per element).  Both epilogues apply
    bias, activation, residual and mask to the same accumulator in the same order: bit-identical."""
    x, wt, b, ref, opers = _conv_inputs(cin, cout, h, w, act, c1, res, mask)
    pk, _, _, ocb = ops.pack_conv3x3(wt.cuda())
    opers += [Operand('w', 'fixed', pk.cpu()), Operand('bias', 'fixed', b),
              Operand('y', 'out', shape=(N, cout, h, w), strided=True, p5=True)]

    def call(lib, p, s):
        a = (p['x'], s['x'], c1 or cin, p.get('x2'), s.get('x2', 0), p['w'], ocb, p['bias'], p.get('res'), s.get('res', 0))
        tail = (p['y'], s['y'], N, cin, cout, h, w, act, None)
        if mask:
            return lib.tg_conv3x3_fwd_masked(*a, p['mask'], s['mask'], *tail)
        return lib.tg_conv3x3_fwd(*a, *tail)
    run_case(lib, Case(f'conv3x3_fwd{"_masked" if mask else ""} {cin}->{cout} {h}x{w} c1={c1} res={res}', opers, call,
                       maxerr('y', ref, act_tol(act))))


@pytest.mark.parametrize('cin,cout,h,w,c1,ks,pool', SPLITK_CASES)
def test_conv3x3_splitk_placements(ops, lib, cin, cout, h, w, c1, ks, pool):
    """tg_conv3x3_splitk_fwd: x / x2 strided, y and the partial sums packed (the ABI has no stride for them); both
    launches address element by element, so every base offset is accepted.  With pool, y is (n, cout, h/2, w/2)."""
    x, wt, b, ref, opers = _conv_inputs(cin, cout, h, w, 2, c1, False, False)
    if pool:
        ref = F.max_pool2d(ref, 2, 2)
    pk, _, _, ocb = ops.pack_conv3x3(wt.cuda())
    opers += [Operand('w', 'fixed', pk.cpu()), Operand('bias', 'fixed', b),
              Operand('partials', 'scratch', shape=(ks * N * cout * h * w,)),
              Operand('y', 'out', shape=tuple(ref.shape))]

    def call(lib, p, s):
        return lib.tg_conv3x3_splitk_fwd(p['x'], s['x'], c1 or cin, p.get('x2'), s.get('x2', 0), p['w'], ocb, p['bias'],
                                         p['y'], N, cin, cout, h, w, 2, ks, p['partials'], 1 if pool else 0, None)
    run_case(lib, Case(f'conv3x3_splitk_fwd {cin}->{cout} {h}x{w} ks={ks} pool={pool}', opers, call,
                       maxerr('y', ref, 1e-5)))


@pytest.mark.parametrize('cin,cout,ho,wo,act,mask', S2_CASES)
def test_conv3x3s2_placements(ops, lib, cin, cout, ho, wo, act, mask):
    """tg_conv3x3s2_fwd (stride 2, x is (n, cin, 2 h_out, 2 w_out)): one store per element at any placement."""
    x = rs(1, (N, cin, 2 * ho, 2 * wo))
    wt = rs(2, (cout, cin, 3, 3)) / (3.0 * cin ** 0.5)
    b = rs(3, (cout,), -0.5, 0.5)
    m = rs(5, (N, cout, ho, wo)) if mask else None
    ref = act_ref(F.conv2d(x.double(), wt.double(), b.double(), stride=2, padding=1), act)
    if mask:
        ref = torch.where(m.double() > 0, ref, torch.zeros_like(ref))
    pk = ops.pack_conv3x3(wt.cuda(), ocb=64)[0]
    opers = [Operand('x', 'in', x, strided=True)] + ([Operand('mask', 'in', m, strided=True)] if mask else []) + \
        [Operand('w', 'fixed', pk.cpu()), Operand('bias', 'fixed', b),
         Operand('y', 'out', shape=(N, cout, ho, wo), strided=True, p5=True)]

    def call(lib, p, s):
        return lib.tg_conv3x3s2_fwd(p['x'], s['x'], p['w'], p['bias'], p.get('mask'), s.get('mask', 0), p['y'], s['y'],
                                    N, cin, cout, ho, wo, act, None)
    run_case(lib, Case(f'conv3x3s2_fwd {cin}->{cout} out {ho}x{wo} mask={mask}', opers, call, maxerr('y', ref, 1e-5)))


# ======================================================================================================================
# tg_conv3x3_wino.hip
# ======================================================================================================================
@pytest.mark.parametrize('cin,cout,h,w,act,c1,res,mask', WINO_CASES)
def test_conv3x3_wino_placements(ops, lib, cin, cout, h, w, act, c1, res, mask):
    """tg_conv3x3_wino_fwd (two-source, residual, mask): accepts every placement; float2 epilogue where w and h * w
    are even and y / res / mask are 8-byte aligned with even strides (P2 and P4 keep it, P1 and P3 do not), one
    access per element otherwise.  Same inverse transform and epilogue order in both: bit-identical."""
    x, wt, b, ref, opers = _conv_inputs(cin, cout, h, w, act, c1, res, mask)
    u = ops.pack_conv3x3_wino(wt.cuda())
    opers += [Operand('u', 'fixed', u.cpu()), Operand('bias', 'fixed', b),
              Operand('y', 'out', shape=(N, cout, h, w), strided=True, p5=True)]

    def call(lib, p, s):
        return lib.tg_conv3x3_wino_fwd(p['x'], s['x'], c1 or cin, p.get('x2'), s.get('x2', 0), p['u'], p['bias'],
                                       p.get('res'), s.get('res', 0), p.get('mask'), s.get('mask', 0), p['y'], s['y'],
                                       N, cin, cout, h, w, act, None)
    run_case(lib, Case(f'conv3x3_wino_fwd {cin}->{cout} {h}x{w} c1={c1} res={res} mask={mask}', opers, call,
                       maxerr('y', ref, act_tol(act))))


@pytest.mark.parametrize('cin,cout,h,w,act,fuse', WINO_FUSED_CASES)
def test_conv3x3_wino_fused_placements(ops, lib, cin, cout, h, w, act, fuse):
    """tg_conv3x3_wino_fused_fwd: POOL (y is (n, cout, h/2, w/2), one store per element) and UP2 (x is the
    (n, cin, h/2, w/2) source of the bilinear x2 in front of the conv)."""
    wt = rs(2, (cout, cin, 3, 3)) / (3.0 * cin ** 0.5)
    b = rs(3, (cout,), -0.5, 0.5)
    if fuse == 2:
        x = rs(1, (N, cin, h // 2, w // 2))
        xin = F.interpolate(x.double(), scale_factor=2, mode='bilinear', align_corners=False)
    else:
        x = rs(1, (N, cin, h, w))
        xin = x.double()
    ref = act_ref(F.conv2d(xin, wt.double(), b.double(), padding=1), act)
    if fuse == 1:
        ref = F.max_pool2d(ref, 2, 2)
    u = ops.pack_conv3x3_wino(wt.cuda())
    opers = [Operand('x', 'in', x, strided=True), Operand('u', 'fixed', u.cpu()), Operand('bias', 'fixed', b),
             Operand('y', 'out', shape=tuple(ref.shape), strided=True, p5=True)]

    def call(lib, p, s):
        return lib.tg_conv3x3_wino_fused_fwd(p['x'], s['x'], p['u'], p['bias'], p['y'], s['y'], N, cin, cout, h, w, act,
                                             fuse, None)
    run_case(lib, Case(f'conv3x3_wino_fused_fwd {"POOL" if fuse == 1 else "UP2"} {cin}->{cout} {h}x{w}', opers, call,
                       maxerr('y', ref, act_tol(act))))


# ======================================================================================================================
# tg_conv3x3_small.hip
# ======================================================================================================================
def small_vec_ok(info, w, names=('x', 'y')):
    """small_launch's vec_ok: w % 4 == 0, 16-byte aligned x and y, strides % 4 == 0."""
    return w % 4 == 0 and all(al(info, k, 4) for k in names)


@pytest.mark.parametrize('cin,cout,h,w,act,up', SMALL_CASES)
def test_conv3x3_small_placements(ops, lib, cin, cout, h, w, act, up):
    """tg_conv3x3_small_fwd with and without up_src: every placement is accepted; where w % 4 == 0 and x / y are
    16-byte aligned with strides % 4 == 0 a 16-byte form runs, else the scalar form (up_src is read element by
    element, packed, in all of them).

    SMALL_KS -- the one form that sums differently: without up_src and with fewer than 512 tiles the 16-byte form is
    conv3x3_small_ks_kernel, whose four waves each sum a quarter of the input channels before the partial sums are
    added; the scalar form (and conv3x3_small_v2_kernel, which runs with up_src) walks the channels in order.  A
    placement that moves such a case off the ks form therefore keeps only the fp64 bound; with up_src the two forms
    (v2 and scalar) accumulate in the same order and bit-identity is asserted."""
    from oracle import tecogan_oracle as O
    x = rs(1, (N, cin, h, w))
    wt = rs(2, (cout, cin, 3, 3)) / (3.0 * cin ** 0.5)
    b = rs(3, (cout,), -0.5, 0.5)
    ref = act_ref(F.conv2d(x.double(), wt.double(), b.double(), padding=1), act)
    opers = [Operand('x', 'in', x, strided=True)]
    mode, s_ = 0, 1
    if up:
        deg, s_ = up
        src = rs(6, (N, cout, h // s_, w // s_), 0, 1)
        ref = ref + O.upsample(src, s_, deg).double()
        mode = ops.UP_MODE[deg]
        opers.append(Operand('up_src', 'in', src))
    opers += [Operand('w', 'fixed', wt), Operand('bias', 'fixed', b),
              Operand('y', 'out', shape=(N, cout, h, w), strided=True, p5=True)]

    def call(lib, p, s):
        return lib.tg_conv3x3_small_fwd(p['x'], s['x'], p['w'], p['bias'], p.get('up_src'), mode, s_, p['y'], s['y'], N,
                                        cin, cout, h, w, act, None)
    ks_at_p0 = (not up) and w % 4 == 0           # (every case here has fewer than 512 tiles)
    run_case(lib, Case(f'conv3x3_small_fwd {cin}->{cout} {h}x{w} act={act} up={up}', opers, call,
                       maxerr('y', ref, act_tol(act)),
                       same_bits=lambda info: not ks_at_p0 or small_vec_ok(info, w)))


@pytest.mark.parametrize('cin,cout,h,w,act', SMALL_RES_CASES)
def test_conv3x3_small_res_placements(lib, cin, cout, h, w, act):
    """tg_conv3x3_small_fwd_res has no scalar form: TG_E_ARG unless w % 4 == 0 and x, res, y are 16-byte aligned with
    strides % 4 == 0 (P4 and, where 3 h w % 4 == 0, P5 pass; P1, P2, P3 are refused and nothing is written)."""
    x = rs(1, (N, cin, h, w))
    wt = rs(2, (cout, cin, 3, 3)) / (3.0 * cin ** 0.5)
    b = rs(3, (cout,), -0.5, 0.5)
    r = rs(4, (N, cout, h, w))
    ref = act_ref(F.conv2d(x.double(), wt.double(), b.double(), padding=1), act) + r.double()
    opers = [Operand('x', 'in', x, strided=True), Operand('res', 'in', r, strided=True), Operand('w', 'fixed', wt),
             Operand('bias', 'fixed', b), Operand('y', 'out', shape=(N, cout, h, w), strided=True, p5=True)]

    def call(lib, p, s):
        return lib.tg_conv3x3_small_fwd_res(p['x'], s['x'], p['w'], p['bias'], p['res'], s['res'], p['y'], s['y'], N, cin,
                                            cout, h, w, act, None)
    run_case(lib, Case(f'conv3x3_small_fwd_res {cin}->{cout} {h}x{w}', opers, call, maxerr('y', ref, act_tol(act)),
                       expect=lambda info: 0 if small_vec_ok(info, w, ('x', 'res', 'y')) else TG_E_ARG))


@pytest.mark.parametrize('cin,cout,h,w,mask', FEWIN_CASES)
def test_conv3x3_fewin_placements(lib, cin, cout, h, w, mask):
    """tg_conv3x3_fewin_fwd (cin <= 4, any cout, optional ReLU mask): 16-byte accesses only, so TG_E_ARG unless
    w % 4 == 0 and x, mask, y are 16-byte aligned with strides % 4 == 0."""
    x = rs(1, (N, cin, h, w))
    wt = rs(2, (cout, cin, 3, 3)) / (3.0 * cin ** 0.5)
    m = rs(5, (N, cout, h, w)) if mask else None
    ref = F.conv2d(x.double(), wt.double(), None, padding=1)
    if mask:
        ref = torch.where(m.double() > 0, ref, torch.zeros_like(ref))
    opers = [Operand('x', 'in', x, strided=True)] + ([Operand('mask', 'in', m, strided=True)] if mask else []) + \
        [Operand('w', 'fixed', wt), Operand('y', 'out', shape=(N, cout, h, w), strided=True, p5=True)]

    def call(lib, p, s):
        return lib.tg_conv3x3_fewin_fwd(p['x'], s['x'], p['w'], p.get('mask'), s.get('mask', 0), p['y'], s['y'], N, cin,
                                        cout, h, w, None)
    names = ('x', 'mask', 'y') if mask else ('x', 'y')
    run_case(lib, Case(f'conv3x3_fewin_fwd {cin}->{cout} {h}x{w} mask={mask}', opers, call, maxerr('y', ref, 1e-5),
                       expect=lambda info: 0 if small_vec_ok(info, w, names) else TG_E_ARG))


# ======================================================================================================================
# tg_convt3x3s2_mfma.hip, tg_convt3x3s2_wino.hip
# ======================================================================================================================
@pytest.mark.parametrize('cin,cout,h,w', CONVT_CASES)
def test_convt3x3s2_placements(ops, lib, cin, cout, h, w):
    """tg_convt3x3s2_fwd: x anywhere (4-byte buffer loads); y leaves as float2 pairs at even offsets of an image, so
    the launcher wants y 8-byte aligned and y_nstride even, TG_E_ARG otherwise (P1 and P3 on y)."""
    x = rs(1, (N, cin, h, w))
    wt = rs(2, (cin, cout, 3, 3)) / (1.5 * cin ** 0.5)
    b = rs(3, (cout,), -0.5, 0.5)
    ref = torch.relu(F.conv_transpose2d(x.double(), wt.double(), b.double(), stride=2, padding=1, output_padding=1))
    pk = ops.pack_conv3x3(wt.cuda(), transposed=True)[0]
    opers = [Operand('x', 'in', x, strided=True), Operand('w', 'fixed', pk.cpu()), Operand('bias', 'fixed', b),
             Operand('y', 'out', shape=(N, cout, 2 * h, 2 * w), strided=True, p5=True)]

    def call(lib, p, s):
        return lib.tg_convt3x3s2_fwd(p['x'], s['x'], p['w'], p['bias'], p['y'], s['y'], N, cin, cout, h, w, 1, None)
    run_case(lib, Case(f'convt3x3s2_fwd {cin}->{cout} {h}x{w}', opers, call, maxerr('y', ref, 1e-5),
                       expect=lambda info: 0 if al(info, 'y', 2) else TG_E_ARG))


def _z_case(ops, cin, cout, cz, h, w):
    x = rs(1, (N, cin, h, w))
    wt = rs(2, (cin, cout, 3, 3)) / (1.5 * cin ** 0.5)
    b = rs(3, (cout,), -0.5, 0.5)
    wo = rs(4, (cz, cout, 3, 3)) / (3.0 * cout ** 0.5)
    up = torch.relu(F.conv_transpose2d(x.double(), wt.double(), b.double(), stride=2, padding=1, output_padding=1))
    ref = torch.einsum('octk,nchw->ntkohw', wo.double().reshape(cz, cout, 3, 3), up).reshape(N, 9 * cz, 2 * h, 2 * w)
    pk = ops.pack_conv3x3(wt.cuda(), transposed=True)[0]
    wz = ops.convt_pack_wz(wo.cuda())
    # z is (n, 32, 2h, 2w) of which the first 9 cz planes are written: the other planes are a gap that must survive
    z = Operand('z', 'out', shape=(N, 9 * cz, 2 * h, 2 * w), strided=True, packed=32 * 4 * h * w)
    return x, b, pk, wz, ref, z


@pytest.mark.parametrize('form', Z_FORMS)
@pytest.mark.parametrize('cin,cout,cz,h,w', CONVT_Z_CASES)
def test_convt3x3s2_z_placements(ops, lib, cin, cout, cz, h, w, form):
    """tg_convt3x3s2_z_fwd_form, every form it still accepts: 8-byte buffer stores into z, so z 8-byte aligned and
    z_nstride even or TG_E_ARG; the planes past 9 cz of each image are never touched."""
    x, b, pk, wz, ref, z = _z_case(ops, cin, cout, cz, h, w)
    opers = [Operand('x', 'in', x, strided=True), Operand('w', 'fixed', pk.cpu()), Operand('bias', 'fixed', b),
             Operand('wz', 'fixed', wz.cpu()), z]

    def call(lib, p, s):
        return lib.tg_convt3x3s2_z_fwd_form(p['x'], s['x'], p['w'], p['bias'], p['wz'], cz, p['z'], s['z'], N, cin, cout,
                                            h, w, 1, form, None)
    run_case(lib, Case(f'convt3x3s2_z_fwd_form({form}) {cin}->{cout} cz={cz} {h}x{w}', opers, call,
                       maxerr('z', ref, 1e-5), expect=lambda info: 0 if al(info, 'z', 2) else TG_E_ARG))


@pytest.mark.parametrize('split', Z_WINO_SPLITS)
@pytest.mark.parametrize('cin,cout,cz,h,w', CONVT_Z_CASES)
def test_convt3x3s2_z_wino_placements(ops, lib, cin, cout, cz, h, w, split):
    """tg_convt3x3s2_z_wino_fwd: the planes leave as 16-byte buffer stores (8-byte in the last column of an odd-width
    map) at even float offsets of an image.  The launcher checked neither the base nor the stride of z; it now has
    the direct form's contract (8-byte aligned z, even z_nstride, TG_E_ARG otherwise), which P1 and P3 on z assert."""
    x, b, pk, wz, ref, z = _z_case(ops, cin, cout, cz, h, w)
    wa = ops.convt_pack_wino(pk, cin, cout)
    opers = [Operand('x', 'in', x, strided=True), Operand('wa', 'fixed', wa.cpu()), Operand('bias', 'fixed', b),
             Operand('wz', 'fixed', wz.cpu()), z]

    def call(lib, p, s):
        return lib.tg_convt3x3s2_z_wino_fwd(p['x'], s['x'], p['wa'], p['bias'], p['wz'], cz, p['z'], s['z'], N, cin, cout,
                                            h, w, 1, split, None)
    run_case(lib, Case(f'convt3x3s2_z_wino_fwd(split {split}) {cin}->{cout} cz={cz} {h}x{w}', opers, call,
                       maxerr('z', ref, 1e-5), expect=lambda info: 0 if al(info, 'z', 2) else TG_E_ARG))


@pytest.mark.parametrize('form', TAIL_FORMS)
@pytest.mark.parametrize('cz,h,w,up', TAIL_CASES)
def test_convout_tail_placements(ops, lib, cz, h, w, up, form):
    """tg_convout_tail_form: form 0 (one pixel per thread) takes every placement; form 1 (four) needs w % 4 == 0 and
    16-byte aligned z / y with strides % 4 == 0, TG_E_SHAPE otherwise; form -1 picks.  z is read as the first 9 cz of
    32 planes per image (the other planes hold the guard NaN here).  Both forms add the taps in the same order."""
    from oracle import tecogan_oracle as O
    z = rs(1, (N, 9 * cz, h, w))
    b = rs(2, (cz,), -0.5, 0.5)
    ref = torch.zeros(N, cz, h, w, dtype=torch.float64)
    zp = F.pad(z.double(), (1, 1, 1, 1))
    for ky in range(3):
        for kx in range(3):
            ref += zp[:, (ky * 3 + kx) * cz:(ky * 3 + kx + 1) * cz, ky:ky + h, kx:kx + w]
    ref += b.double().view(1, cz, 1, 1)
    opers = [Operand('z', 'in', z, strided=True, packed=32 * h * w)]
    mode, s_ = 0, 1
    if up:
        deg, s_ = up
        src = rs(3, (N, cz, h // s_, w // s_), 0, 1)
        ref += O.upsample(src, s_, deg).double()
        mode = ops.UP_MODE[deg]
        opers.append(Operand('up_src', 'in', src))
    opers += [Operand('bias', 'fixed', b), Operand('y', 'out', shape=(N, cz, h, w), strided=True, p5=True)]

    def call(lib, p, s):
        return lib.tg_convout_tail_form(p['z'], s['z'], cz, p['bias'], p.get('up_src'), mode, s_, p['y'], s['y'], None, N,
                                        h, w, form, None)
    run_case(lib, Case(f'convout_tail_form({form}) cz={cz} {h}x{w} up={up}', opers, call, maxerr('y', ref, 2e-5),
                       expect=lambda info: TG_E_SHAPE if form == 1 and not small_vec_ok(info, w, ('z', 'y')) else 0))


# ======================================================================================================================
# tg_conv3x3_f16.hip
# ======================================================================================================================
def _h(t):
    return t.to(torch.float16).to(torch.float32)


@pytest.mark.parametrize('c1,c2,h,w', F16_PACK_CASES)
def test_f16_pack_input_placements(lib, c1, c2, h, w):
    """tg_conv3x3_f16_pack_input: the fp32 NCHW sources are read element by element at any base and stride; the fp16
    channels-last destination is written 16 bytes at a time and must be 16-byte aligned (TG_E_ARG: P1 and P2 are 4
    and 8 bytes).  Exact: the rounded concatenation, bit for bit."""
    x1 = rs(1, (N, c1, h, w)) * 0.7
    x2 = rs(2, (N, c2, h, w)) * 300.0 if c2 else None
    exp = torch.zeros(N, h, w, 64, dtype=torch.float16)
    exp[..., :c1 + c2] = (torch.cat([x1, x2], 1) if c2 else x1).permute(0, 2, 3, 1).to(torch.float16)
    opers = [Operand('x1', 'in', x1, strided=True)] + ([Operand('x2', 'in', x2, strided=True)] if c2 else []) + \
        [Operand('y', 'out', shape=(N, h, w, 64), dtype=torch.float16)]

    def call(lib, p, s):
        return lib.tg_conv3x3_f16_pack_input(p['x1'], s['x1'], c1, p.get('x2'), s.get('x2', 0), c2, p['y'], N, h, w, None)

    def verify(outs):
        return [('y (halves that differ)', float((outs['y'].view(torch.int16) != exp.view(torch.int16)).sum()), 0.0)]
    run_case(lib, Case(f'conv3x3_f16_pack_input {c1}+{c2} {h}x{w}', opers, call, verify,
                       expect=lambda info: 0 if info['y'][0] % 4 == 0 else TG_E_ARG))


@pytest.mark.parametrize('h,w,relu,skip', F16_CONV_CASES)
def test_conv3x3_f16_placements(ops, lib, h, w, relu, skip):
    """tg_conv3x3_f16_fwd takes no strides and wants every pointer 16-byte aligned: P1 and P2 on x, res or y are
    TG_E_ARG and nothing is written; P0 inside the arena (NaN all around the packed images) is within the fp16
    file's derived bound."""
    import fp16_fixture as FX
    wt = _h(rs(2, (64, 64, 3, 3)) / (3.0 * 8))
    b = rs(3, (64,), -0.5, 0.5)
    x, r = _h(rs(1, (N, 64, h, w))), _h(rs(4, (N, 64, h, w)))
    E, S = FX.layer_ref(x, wt, b, relu, r if skip else None)
    bound = FX.bound_f16_out(E, S)
    wp = ops.f16_pack_weights(wt.cuda().contiguous())
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().to(torch.float16)      # noqa: E731
    opers = [Operand('x', 'in', nhwc(x))] + ([Operand('res', 'in', nhwc(r))] if skip else []) + \
        [Operand('w', 'fixed', wp.cpu()), Operand('bias', 'fixed', b),
         Operand('y', 'out', shape=(N, h, w, 64), dtype=torch.float16)]

    def call(lib, p, s):
        return lib.tg_conv3x3_f16_fwd(p['x'], p['w'], p['bias'], p.get('res'), p['y'], N, 64, 64, h, w, 1 if relu else 0, None)

    def verify(outs):
        d = (outs['y'].double().permute(0, 3, 1, 2) - E).abs()
        return [('y (share of the derived bound)', (d / bound).max().item(), 1.0)]
    names = ('x', 'res', 'y') if skip else ('x', 'y')
    run_case(lib, Case(f'conv3x3_f16_fwd {h}x{w} relu={relu} skip={skip}', opers, call, verify,
                       expect=lambda info: 0 if all(info[k][0] % 4 == 0 for k in names) else TG_E_ARG))


@pytest.mark.parametrize('h,w,relu', F16_CONVT_CASES)
def test_convt3x3s2_f16_placements(ops, lib, h, w, relu):
    """tg_convt3x3s2_f16_fwd: x fp16 channels-last, 16-byte aligned (TG_E_ARG); y fp32 NCHW written as float2 pairs:
    8-byte aligned, y_nstride even (TG_E_ARG) and at least one image (TG_E_SHAPE)."""
    import fp16_fixture as FX
    wt = _h(rs(2, (64, 64, 3, 3)) / (1.5 * 8))
    b = rs(3, (64,), -0.5, 0.5)
    x = _h(rs(1, (N, 64, h, w)))
    E, S = FX.layer_ref(x, wt, b, relu, transposed=True)
    bound = FX.bound_f32_out(E, S)
    wp = ops.f16_pack_weights(wt.cuda().contiguous(), transposed=True)
    opers = [Operand('x', 'in', x.permute(0, 2, 3, 1).contiguous().to(torch.float16)), Operand('w', 'fixed', wp.cpu()),
             Operand('bias', 'fixed', b), Operand('y', 'out', shape=(N, 64, 2 * h, 2 * w), strided=True, p5=True)]

    def call(lib, p, s):
        return lib.tg_convt3x3s2_f16_fwd(p['x'], p['w'], p['bias'], p['y'], s['y'], N, 64, 64, h, w, 1 if relu else 0, None)

    def verify(outs):
        return [('y (share of the derived bound)', ((outs['y'].double() - E).abs() / bound).max().item(), 1.0)]
    run_case(lib, Case(f'convt3x3s2_f16_fwd {h}x{w} relu={relu}', opers, call, verify,
                       expect=lambda info: 0 if info['x'][0] % 4 == 0 and al(info, 'y', 2) else TG_E_ARG))


# ======================================================================================================================
# the glue kernels (tg_warp.hip) and the discriminator's strided conv
# ======================================================================================================================
@pytest.mark.parametrize('c,h,w', WARP_CASES)
def test_backward_warp_placements(lib, c, h, w):
    """tg_backward_warp_fwd takes no strides and addresses element by element: every base offset is accepted."""
    from oracle import tecogan_oracle as O
    x, flow = rs(1, (N, c, h, w), 0, 1), rs(2, (N, 2, h, w), -3, 3)
    ref = O.backward_warp(x, flow).double()
    opers = [Operand('x', 'in', x), Operand('flow', 'in', flow), Operand('y', 'out', shape=(N, c, h, w))]
    run_case(lib, Case(f'backward_warp_fwd c={c} {h}x{w}', opers,
                       lambda lib, p, s: lib.tg_backward_warp_fwd(p['x'], p['flow'], p['y'], N, c, h, w, None),
                       maxerr('y', ref, 5e-6)))


@pytest.mark.parametrize('deg,s,h,w', FLOWUP_CASES)
def test_flowup_warp_s2d_placements(ops, lib, deg, s, h, w):
    """tg_flowup_warp_s2d_fwd: lr_flow, hr_prev and hr_flow_out packed (no strides in the ABI), out strided.  The
    gathers are buffer loads bounded per image at any 4-byte offset; out leaves as 16-byte buffer stores only where
    w % 4 == 0 and out is 16-byte aligned with out_nstride % 4 == 0, else element by element."""
    from oracle import tecogan_oracle as O
    fh, fw = h // 8 * 8, w // 8 * 8
    lr_flow = rs(1, (N, 2, fh, fw), -5, 5)
    hr_prev = rs(2, (N, 3, s * h, s * w), 0, 1)
    hr_flow = s * O.upsample(O.reflect_pad_br(lr_flow, h - fh, w - fw), s, deg)
    ref = O.space_to_depth(O.backward_warp(hr_prev, hr_flow), s).double()
    opers = [Operand('lr_flow', 'in', lr_flow), Operand('hr_prev', 'in', hr_prev),
             Operand('out', 'out', shape=(N, s * s * 3, h, w), strided=True, p5=True),
             Operand('hr_flow', 'out', shape=(N, 2, s * h, s * w))]

    def call(lib, p, s_):
        return lib.tg_flowup_warp_s2d_fwd(p['lr_flow'], fh, fw, p['hr_prev'], p['out'], s_['out'], p['hr_flow'], N, 3, h, w,
                                          s, ops.UP_MODE[deg], None)

    def verify(outs):
        return [('hr_flow', (outs['hr_flow'].double() - hr_flow.double()).abs().max().item(), 2e-5),
                ('out', (outs['out'].double() - ref).abs().max().item(), 5e-5)]
    run_case(lib, Case(f'flowup_warp_s2d_fwd {deg} x{s} {h}x{w}', opers, call, verify))


@pytest.mark.parametrize('c,h,w,s', S2D_CASES)
def test_space_to_depth_placements(lib, c, h, w, s):
    """tg_space_to_depth (y_nstride): the 16-byte form where s is 2 or 4, w % 4s == 0, x and y are 16-byte aligned
    and y_nstride % 4 == 0, the element form otherwise.  A permutation: exact."""
    from oracle import tecogan_oracle as O
    x = rs(1, (N, c, h, w))
    ref = O.space_to_depth(x, s)
    opers = [Operand('x', 'in', x), Operand('y', 'out', shape=tuple(ref.shape), strided=True, p5=True)]

    def verify(outs):
        return [('y (elements that differ)', float((outs['y'] != ref).sum()), 0.0)]
    run_case(lib, Case(f'space_to_depth c={c} {h}x{w} s={s}', opers,
                       lambda lib, p, s_: lib.tg_space_to_depth(p['x'], p['y'], s_['y'], N, c, h, w, s, None), verify))


@pytest.mark.parametrize('c,h,w,s,deg', UPSAMPLE_CASES)
def test_upsample_placements(ops, lib, c, h, w, s, deg):
    """tg_upsample_fwd (no strides): bilinear x2 on an even width with a 16-byte aligned y runs the 2 x 4-patch form
    (16-byte stores), everything else the element form; same taps, weights and expression."""
    from oracle import tecogan_oracle as O
    x = rs(1, (N, c, h, w))
    ref = 3.0 * O.upsample(x, s, deg).double()
    opers = [Operand('x', 'in', x), Operand('y', 'out', shape=(N, c, s * h, s * w))]
    run_case(lib, Case(f'upsample_fwd {deg} x{s} c={c} {h}x{w}', opers,
                       lambda lib, p, s_: lib.tg_upsample_fwd(p['x'], p['y'], N * c, h, w, s, ops.UP_MODE[deg], 3.0, None),
                       maxerr('y', ref, 8e-6 if deg == 'BD' else 4e-6)))


@pytest.mark.parametrize('c,h,w', MAXPOOL_CASES)
def test_maxpool2_placements(lib, c, h, w):
    """tg_maxpool2_fwd (no strides): two float4 loads and one float2 store per thread where w % 4 == 0 and x, y are
    16-byte aligned, the element form otherwise.  Exact."""
    x = rs(1, (N, c, h, w))
    ref = F.max_pool2d(x, 2, 2)
    opers = [Operand('x', 'in', x), Operand('y', 'out', shape=tuple(ref.shape))]

    def verify(outs):
        return [('y (elements that differ)', float((outs['y'] != ref).sum()), 0.0)]
    run_case(lib, Case(f'maxpool2_fwd c={c} {h}x{w}', opers,
                       lambda lib, p, s_: lib.tg_maxpool2_fwd(p['x'], p['y'], N * c, h, w, None), verify))


@pytest.mark.parametrize('ci,co,h,w', CONV4_CASES)
def test_conv4x4s2_placements(ops, lib, ci, co, h, w):
    """tg_conv4x4s2_fwd takes no strides; x is read and y written element by element.  The small-map forms that split
    the input channels add the partial sums in a second launch, 16 bytes per thread, over y and the workspace: the
    launcher let any pointer through to it and now returns TG_E_ARG unless both are 16-byte aligned."""
    g = torch.Generator().manual_seed(11)
    x = torch.randn(N, ci, h, w, generator=g)
    wt = torch.randn(co, ci, 4, 4, generator=g) * 0.05
    ref = F.conv2d(x.double(), wt.double(), None, 2, 1)
    assert lib.tg_conv4x4s2_supported(N, ci, co, h, w)
    pf, _ = ops.pack_conv4x4s2(wt.cuda())
    wsf = lib.tg_conv4x4s2_workspace_floats(N, ci, co, h, w, 0)
    opers = [Operand('x', 'in', x), Operand('w', 'fixed', pf.cpu()), Operand('y', 'out', shape=tuple(ref.shape))]
    if wsf:
        opers.append(Operand('workspace', 'scratch', shape=(wsf,)))

    def call(lib, p, s):
        return lib.tg_conv4x4s2_fwd(p['x'], p['w'], p['y'], p.get('workspace'), N, ci, co, h, w, None)

    def expect(info):
        return 0 if not wsf or (info['y'][0] % 4 == 0 and info['workspace'][0] % 4 == 0) else TG_E_ARG
    run_case(lib, Case(f'conv4x4s2_fwd {ci}->{co} {h}x{w} split={bool(wsf)}', opers, call,
                       maxerr('y', ref, 2e-5 * ref.abs().max().item()), expect=expect))
