"""CPU: what tests/test_hip_placement.py stands on, without a GPU.

1. tests/placement.py (Arena) is proved with plain torch stand-ins for a kernel: a correct one passes; one that writes
   an element past a row, one that ignores the batch stride and one that reads a neighbour are each caught, with the
   operand named.
2. The host-side choices of the launchers that depend on shape or placement are restated here in Python, next to the
   names of the code they restate, and the GPU case tables are checked to reach every value of each -- the case table
   is only as good as the forms it reaches.
3. The batch-stride contract and the alignment gates this file's companion found missing are checked through the C
   ABI with host addresses (the checks come before any launch), the pattern of tests/test_abi_cpu.py."""
import ctypes

import numpy as np
import pytest
import torch

from tests import test_hip_placement as G
from tests.placement import Arena, PLACEMENTS, pattern, extent_floats


# ======================================================================================================================
# 1. the arena, with CPU stand-ins for a kernel
# ======================================================================================================================
def standin(arena, x, y, c, h, w, bug=None):
    """y[b, ch, r, :] = 2 * x[b, ch, r, :] the way a kernel does it: flat indices into the one allocation, from base
    addresses and batch strides.  bug: None | 'past_row' | 'ignores_nstride' | 'reads_neighbour'."""
    mem = arena.words.view(torch.float32)
    xo, yo = x._arena_op['base'], y._arena_op['base']
    xns, yns = Arena.nstride(x), Arena.nstride(y)
    if bug == 'ignores_nstride':
        yns = c * h * w                                    # the packed stride where y_nstride was meant
    for b in range(x.shape[0]):
        for ch in range(c):
            for r in range(h):
                src = xo + b * xns + (ch * h + r) * w
                dst = yo + b * yns + (ch * h + r) * w
                row = 2.0 * mem[src:src + w]
                if bug == 'reads_neighbour' and b == x.shape[0] - 1 and ch == c - 1 and r == h - 1:
                    row = row + 0.0 * mem[src + w]         # one element past the last row of the last image, weight 0
                mem[dst:dst + w] = row
                if bug == 'past_row' and b == 0 and ch == c - 1 and r == h - 1:
                    mem[dst + w] = 1.0                     # a ragged tile's store, one element past the row


def _arena_with(x, y_place):
    a = Arena('cpu', margin_floats=1024, slots=3)
    xv = a.place(x, offset_floats=1, nstride=x[0].numel() + 8, name='x')
    other = a.place(torch.arange(12, dtype=torch.float32), name='bias')
    yv = a.out(tuple(x.shape), name='y', **y_place)
    return a, xv, other, yv


X = torch.arange(2 * 3 * 4 * 5, dtype=torch.float32).reshape(2, 3, 4, 5) / 7.0


@pytest.mark.parametrize('y_place', [dict(), dict(offset_floats=1), dict(nstride=60 + 1), dict(nstride=60 + 8),
                                     dict(nstride=(3 + 3) * 20)])
def test_arena_passes_a_correct_stand_in(y_place):
    a, xv, other, yv = _arena_with(X, y_place)
    assert torch.equal(xv, X) and xv.data_ptr() % 64 == 4 and yv.data_ptr() % 64 == 4 * y_place.get('offset_floats', 0)
    assert Arena.nstride(xv) == 68 and Arena.nstride(yv) == y_place.get('nstride', 60)
    a.check(outputs_untouched=True)                      # nothing launched yet
    with pytest.raises(AssertionError, match='never written'):
        a.finite(yv)
    standin(a, xv, yv, 3, 4, 5)
    a.check()
    a.finite(yv)
    assert torch.equal(yv, 2.0 * X)
    with pytest.raises(AssertionError, match='nearest operand: y'):
        a.check(outputs_untouched=True)                  # ... and a refusal that did launch would show


def test_arena_margins_are_at_least_the_largest_operand_and_hold_the_pattern():
    a, xv, other, yv = _arena_with(X, dict(nstride=68))
    words = a.words.numpy()
    spans = sorted((op['base'], op['base'] + op['words'], op['slot']) for op in a.ops)
    largest = max(hi - lo for lo, hi, _ in spans)
    assert spans[0][0] >= largest and a.total - spans[-1][1] >= largest
    for (_, hi0, _), (lo1, _, _) in zip(spans, spans[1:]):
        assert lo1 - hi0 >= largest
    owned = np.zeros(a.total, dtype=bool)
    for op in a.ops:
        for b in range(op['n']):
            owned[op['base'] + b * op['ns_words']:op['base'] + b * op['ns_words'] + op['per_words']] = True
    guards = words[~owned]
    assert ((guards & ~0xFF) == pattern(0)).all()          # every word no operand owns is the quiet NaN with the payload
    assert np.isnan(guards.view(np.float32)).all() and (words[owned & ~a.free].view(np.float32) == a.expect[owned & ~a.free].view(np.float32)).all()
    gap = words[a.ops[0]['base'] + 60:a.ops[0]['base'] + 68]
    assert (gap == pattern(1)).all()                       # the gap between x's images carries x's slot
    assert pattern(1) != 0x7FC00000 and (pattern(1) & 0x7FC00000) == 0x7FC00000      # not the NaN hardware produces
    with pytest.raises(AssertionError, match='do not fit the margin'):
        a.place(torch.zeros(2000), name='too large')       # an operand may not exceed the margin
    assert extent_floats((2, 3, 4, 5), 68) == 68 + 60 and extent_floats((12,)) == 12


def test_arena_catches_a_write_one_element_past_a_row():
    a, xv, other, yv = _arena_with(X, dict(nstride=68))
    standin(a, xv, yv, 3, 4, 5, bug='past_row')
    with pytest.raises(AssertionError) as e:
        a.check()
    msg = str(e.value)
    assert 'nearest operand: y' in msg and 'word +60 from the base of y' in msg and 'gap behind image 0' in msg, msg
    assert '0x3F800000' in msg                             # the stray 1.0f, shown as the word it is


def test_arena_catches_a_kernel_that_ignores_the_batch_stride():
    a, xv, other, yv = _arena_with(X, dict(nstride=68))
    standin(a, xv, yv, 3, 4, 5, bug='ignores_nstride')
    with pytest.raises(AssertionError) as e:
        a.check()                                          # image 1 began 8 floats early: the gap was written
    assert 'nearest operand: y' in str(e.value) and 'gap behind image 0' in str(e.value), str(e.value)
    with pytest.raises(AssertionError, match=r'y\[1, 2, 2, 2\] was never written'):
        a.finite(yv)                                       # ... and the last 8 elements of image 1 never were


def test_arena_catches_a_read_of_a_neighbour_and_names_the_operand_it_was_read_from():
    a, xv, other, yv = _arena_with(X, dict())
    standin(a, xv, yv, 3, 4, 5, bug='reads_neighbour')
    a.check()                                              # nothing was WRITTEN out of place
    with pytest.raises(AssertionError) as e:
        a.finite(yv)
    assert 'the kernel read outside x' in str(e.value) and 'y[1, 2, 3, 0]' in str(e.value), str(e.value)


def test_arena_notices_a_changed_input_and_tells_a_computed_nan_from_a_guard():
    a, xv, other, yv = _arena_with(X, dict())
    standin(a, xv, yv, 3, 4, 5)
    other[3] = 5.0                                         # a launch may not write a foreign operand
    with pytest.raises(AssertionError, match='nearest operand: bias'):
        a.check()
    yv[0, 0, 0, 0] = float('inf') - float('inf')           # the NaN arithmetic makes: empty payload
    with pytest.raises(AssertionError, match='not a guard word'):
        a.finite(yv)


def test_arena_places_sixteen_bit_operands():
    a = Arena('cpu', margin_floats=512, slots=2)
    t = (torch.arange(2 * 3 * 64, dtype=torch.float32) / 16).reshape(2, 3, 64).to(torch.float16)
    v = a.place(t, offset_floats=4, name='x16')
    y = a.out((2, 3, 64), dtype=torch.float16, name='y16')
    assert torch.equal(v, t) and v.data_ptr() % 64 == 16
    with pytest.raises(AssertionError, match='never written'):
        a.finite(y)
    y.copy_(v)
    a.check()
    a.finite(y)


# ======================================================================================================================
# 2. the launchers' host-side choices, restated, and what the GPU case tables reach
# ======================================================================================================================
def cdiv(a, b):
    return (a + b - 1) // b


def aligned(op_info, k):
    """(offset in floats from a 64-byte boundary, batch stride in floats) is aligned to k floats."""
    off, ns = op_info
    return off % k == 0 and ns % k == 0


def placements_of(operand):
    """Every (offset, stride) the GPU test puts `operand` at."""
    return [r for r in (operand.resolve(p) for p in PLACEMENTS) if r is not None]


def y_operand(cout, h, w):
    return G.Operand('y', 'out', shape=(G.N, cout, h, w), strided=True, p5=True)


# ---- tg_conv3x3_mfma.hip ---------------------------------------------------------------------------------------------
# restates: tg_conv3x3_pick_ocb; conv3x3_rows_per_wg (tg_common.h); conv3x3_uses_wg_ksplit / conv3x3_uses_oneshot; the
# variant ladder at the end of conv3x3_impl; `a.vec_ok = ...` in launch_conv and in conv3x3_impl's one-shot branch (the
# same expression at both sites)
def mfma_ocb(cout):
    return 32 if cout <= 32 else 64


def mfma_variant(n, cin, cout, h, w, ksplit=1):
    if mfma_ocb(cout) == 32:
        return 'rows4 ocb32'                       # launch_conv<4, 1, 1>
    if n * h * w >= 200000:
        return 'rows4'                             # launch_conv<4, 1, 2>: the 4-row variant of the 64-channel block
    wg_ks = cdiv(w, 32) * cdiv(h, 2) * cdiv(cout, 64) * n <= 128 and cdiv(cin, 8) >= 6
    if ksplit <= 1 and wg_ks and cout <= 64 and cdiv(cin, 8) <= 8:
        return 'oneshot'                           # conv3x3_oneshot_kernel
    if ksplit <= 1 and wg_ks:
        return 'wg ksplit'                         # launch_conv<1, 2, 1, 2>
    return 'rows2'                                 # launch_conv<2, 2, 1>


def mfma_vec_ok(w, y, res=None, mask=None):
    return w % 4 == 0 and all(aligned(o, 4) for o in (y, res, mask) if o is not None)


def test_mfma_cases_reach_every_variant_both_ocb_and_both_epilogues():
    reached = {}
    for cin, cout, h, w, act, c1, res, mask in G.MFMA_CASES:
        v = mfma_variant(G.N, cin, cout, h, w)
        for place in placements_of(y_operand(cout, h, w)):
            reached.setdefault(v, set()).add((w % 4 == 0, mfma_vec_ok(w, place)))
    for cin, cout, h, w, c1, ks, pool in G.SPLITK_CASES:
        assert 2 <= ks <= cdiv(cin, 8)
        reached.setdefault(mfma_variant(G.N, cin, cout, h, w, ks), set())
    assert set(reached) == {'rows4 ocb32', 'oneshot', 'wg ksplit', 'rows2'}, sorted(reached)
    for v, seen in reached.items():
        # the float4 epilogue and its per-element fallback, both at w % 4 == 0 (where alone the switch is live), and
        # the fallback at a width that never vectorises
        assert {(True, True), (True, False)} <= seen, (v, seen)
    assert any((False, False) in seen for seen in reached.values())
    assert {mfma_ocb(c[1]) for c in G.MFMA_CASES} == {32, 64}
    assert any(c[5] for c in G.MFMA_CASES) and any(c[6] for c in G.MFMA_CASES) and any(c[7] for c in G.MFMA_CASES)
    assert any(not (c[5] or c[6] or c[7]) for c in G.MFMA_CASES)            # plain, two-source, residual, masked
    assert {(51, 64), (27, 64)} <= {c[:2] for c in G.MFMA_CASES}            # the zero-padded K cases
    assert any(c[1] == 48 for c in G.MFMA_CASES) and any(c[:2] == (128, 128) for c in G.MFMA_CASES)
    assert any(c[3] > 32 for c in G.MFMA_CASES)                             # two workgroups in x
    # 'rows4' needs 200 000 pixels per launch: a map of that size is not placed in an arena.  The form differs from
    # 'rows2' in the rows a workgroup covers, not in how it addresses an operand (one kernel template, one epilogue);
    # test_hip_parity.py CONV_CASES runs it:
    assert mfma_variant(3, 64, 64, 300, 260) == 'rows4'


# ---- tg_conv3x3_wino.hip ---------------------------------------------------------------------------------------------
# restates conv3x3_wino_launch: `oc32`, the `tr` search, `a.vec_ok = ...` (al8), `xcd = blocks >= 512`
def wino_geometry(n, cout, h, w):
    oc32 = cout <= 32
    wgw = 64 if oc32 else 32
    tr, best = 1, cdiv(w, wgw) * cdiv(h, 2)
    for cand in (2, 4):
        c = cdiv(w, wgw // cand) * cdiv(h, 2 * cand)
        if c < best:
            best, tr = c, cand
    blocks = cdiv(w, wgw // tr) * cdiv(h, 2 * tr) * cdiv(cout, 64) * n
    return oc32, tr, blocks >= 512


def wino_vec_ok(h, w, y, res=None, mask=None):
    return w % 2 == 0 and (h * w) % 2 == 0 and all(aligned(o, 2) for o in (y, res, mask) if o is not None)


def test_wino_cases_reach_every_tile_arrangement_of_both_workgroup_shapes_and_both_epilogues():
    reached = {}
    for cin, cout, h, w, act, c1, res, mask in G.WINO_CASES:
        oc32, tr, xcd = wino_geometry(G.N, cout, h, w)
        assert not xcd
        for place in placements_of(y_operand(cout, h, w)):
            reached.setdefault((oc32, tr), set()).add((w % 2 == 0, wino_vec_ok(h, w, place)))
    assert set(reached) == {(o, t) for o in (False, True) for t in (1, 2, 4)}, sorted(reached)
    for k, seen in reached.items():
        assert {(True, True), (True, False)} <= seen, (k, seen)          # float2 and per-element at an even width
    assert any((False, False) in seen for seen in reached.values())      # an odd width
    # P2 keeps the float2 epilogue that P1 loses; the direct kernel's float4 epilogue loses both
    y = y_operand(64, 6, 8)
    assert wino_vec_ok(6, 8, y.resolve('P2')) and not wino_vec_ok(6, 8, y.resolve('P1'))
    assert not mfma_vec_ok(8, y.resolve('P2')) and not mfma_vec_ok(8, y.resolve('P1'))
    assert wino_vec_ok(6, 8, y.resolve('P4')) and not wino_vec_ok(6, 8, y.resolve('P3'))
    fused = {(wino_geometry(G.N, c[1], c[2], c[3])[:2], c[5]) for c in G.WINO_FUSED_CASES}
    assert {f for _, f in fused} == {1, 2} and {g[0] for g, _ in fused} == {False, True}
    assert {(51, 64), (27, 64)} <= {c[:2] for c in G.WINO_CASES} and any(c[:2] == (128, 128) for c in G.WINO_CASES)
    assert any(c[1] == 48 for c in G.WINO_CASES) and any(c[4] == 3 for c in G.WINO_CASES)
    # The XCD-banded order (512 or more workgroups) only permutes which workgroup takes which tile; it needs a map far
    # larger than an arena case should be.  It runs in test_hip_parity.py at the 134x320 layer size
    # (test_winograd_full_size_properties, against the direct form) and in every full-size frame test -- NOT in
    # WINO_CASES' (2, 64, 64, 134, 64), which makes 268 workgroups:
    assert wino_geometry(1, 64, 134, 320) == (False, 1, True)
    assert wino_geometry(2, 64, 134, 64) == (False, 1, False)


# ---- tg_convt3x3s2_mfma.hip: tg_convout_tail_form ----------------------------------------------------------------------
# restates `vec_ok` and the form choice of tg_convout_tail_form
def tail_form(form, w, z, y):
    vec_ok = w % 4 == 0 and aligned(z, 4) and aligned(y, 4)
    if form == 1 and not vec_ok:
        return 'TG_E_SHAPE'
    return 4 if form == 1 or (form == -1 and vec_ok) else 1


def test_tail_cases_reach_both_forms_by_the_rule_and_by_request():
    reached = set()
    for cz, h, w, up in G.TAIL_CASES:
        z = G.Operand('z', 'in', shape=(G.N, 9 * cz, h, w), strided=True, packed=32 * h * w)
        y = y_operand(cz, h, w)
        for form in G.TAIL_FORMS:
            for zp in placements_of(z):
                reached.add((form, tail_form(form, w, zp, y.resolve('P0'))))
            for yp in placements_of(y):
                reached.add((form, tail_form(form, w, z.resolve('P0'), yp)))
    assert reached == {(-1, 4), (-1, 1), (0, 1), (1, 4), (1, 'TG_E_SHAPE')}, reached
    assert any(c[2] > 256 for c in G.TAIL_CASES) and any(c[2] % 4 for c in G.TAIL_CASES)     # two workgroups in x; odd


# ---- the other switches the case tables are meant to flip --------------------------------------------------------------
def test_small_conv_cases_reach_its_three_kernels():
    """small_launch: vec_ok && !up_src && (res || blocks < 512) -> the channel-split form; vec_ok -> the 16-byte form;
    else the scalar form (conv3x3_small_ks_kernel / _v2_kernel / _kernel)."""
    reached = set()
    for cin, cout, h, w, act, up in G.SMALL_CASES:
        blocks = cdiv(w, 64) * cdiv(h, 16) * G.N
        assert blocks < 512
        for place in placements_of(y_operand(cout, h, w)):
            vec_ok = w % 4 == 0 and aligned(place, 4)
            reached.add('ks' if vec_ok and not up else 'v2' if vec_ok else 'scalar up' if up else 'scalar')
    assert reached == {'ks', 'v2', 'scalar', 'scalar up'}
    assert any(c[3] > 64 for c in G.SMALL_CASES)


def test_every_case_has_two_images_and_every_strided_operand_sees_every_placement():
    assert G.N == 2
    y = y_operand(48, 6, 8)
    assert [y.resolve(p) for p in PLACEMENTS] == [(0, 2304), (1, 2304), (2, 2304), (0, 2305), (0, 2312), (0, 51 * 48)]
    packed_only = G.Operand('up_src', 'in', shape=(2, 3, 3, 4))
    assert [packed_only.resolve(p) for p in PLACEMENTS] == [(0, 36), (1, 36), (2, 36), None, None, None]
    case = G.Case('t', [G.Operand('x', 'in', shape=(2, 3, 6, 8), strided=True), packed_only,
                        G.Operand('w', 'fixed', shape=(27,)), y], None, None)
    tags = [t for t, _ in case.placements()]
    assert tags == ['x@P1', 'x@P2', 'x@P3', 'x@P4', 'up_src@P1', 'up_src@P2', 'y@P1', 'y@P2', 'y@P3', 'y@P4', 'y@P5',
                    'all@P1', 'all@P2', 'all@P3', 'all@P4']


# ======================================================================================================================
# 3. the contract the launchers now enforce (host addresses: every check comes before any launch)
# ======================================================================================================================
@pytest.fixture(scope='module')
def lib():
    from tecogan_pytorch_amd import _lib
    return _lib.lib()


@pytest.fixture(scope='module')
def host():
    """Four 64-byte aligned host addresses, 64 KiB apart (never dereferenced: the calls below are all refused)."""
    buf = (ctypes.c_char * (5 << 16))()
    a = (ctypes.addressof(buf) + 63) & ~63
    return buf, [a + (i << 16) for i in range(4)]


def test_batch_strides_smaller_than_an_image_are_refused(lib, host):
    """KERNELS.md, "Buffer placement": with n > 1 the images of an operand may not overlap.  Every entry that takes a
    batch stride returns TG_E_SHAPE for a smaller one and says which; n = 1 never looks at the stride."""
    _, (a, b, c, d) = host
    n, cin, cout, h, w = 2, 16, 8, 6, 8
    px, py = cin * h * w, cout * h * w
    E = -1

    def refused(rc, what):
        msg = lib.tg_last_error_string().decode()
        assert rc == E and f'{what}_nstride' in msg and 'one image' in msg, (rc, msg)
    refused(lib.tg_conv3x3_fwd(a, px - 1, cin, None, 0, b, 32, None, None, 0, c, py, n, cin, cout, h, w, 0, None), 'x')
    refused(lib.tg_conv3x3_fwd(a, px, cin, None, 0, b, 32, None, None, 0, c, py - 1, n, cin, cout, h, w, 0, None), 'y')
    refused(lib.tg_conv3x3_fwd(a, 3 * h * w, 3, d, (cin - 3) * h * w - 1, b, 32, None, None, 0, c, py, n, cin, cout, h, w, 0,
                               None), 'x2')
    refused(lib.tg_conv3x3_fwd(a, px, cin, None, 0, b, 32, None, d, py - 1, c, py, n, cin, cout, h, w, 0, None), 'res')
    refused(lib.tg_conv3x3_fwd_masked(a, px, cin, None, 0, b, 32, None, None, 0, d, py - 1, c, py, n, cin, cout, h, w, 0,
                                      None), 'mask')
    # (an absent operand's stride is not looked at: ops.py passes cout * h * w or 0 for a null res / x2)
    refused(lib.tg_conv3x3s2_fwd(a, 4 * px - 1, b, None, None, 0, c, py, n, cin, cout, h, w, 0, None), 'x')
    refused(lib.tg_conv3x3s2_fwd(a, 4 * px, b, None, None, 0, c, py - 1, n, cin, cout, h, w, 0, None), 'y')
    refused(lib.tg_conv3x3_wino_fwd(a, px - 1, cin, None, 0, b, None, None, 0, None, 0, c, py, n, cin, cout, h, w, 0, None), 'x')
    refused(lib.tg_conv3x3_wino_fwd(a, px, cin, None, 0, b, None, d, py - 1, None, 0, c, py, n, cin, cout, h, w, 0, None), 'res')
    refused(lib.tg_conv3x3_wino_fwd(a, px, cin, None, 0, b, None, None, 0, d, py - 1, c, py, n, cin, cout, h, w, 0, None), 'mask')
    refused(lib.tg_conv3x3_wino_fwd(a, px, cin, None, 0, b, None, None, 0, None, 0, c, py - 1, n, cin, cout, h, w, 0, None), 'y')
    # fused: POOL writes (cout, h/2, w/2) per image, UP2 reads (cin, h/2, w/2)
    refused(lib.tg_conv3x3_wino_fused_fwd(a, px, b, None, c, py // 4 - 1, n, cin, cout, h, w, 0, 1, None), 'y')
    refused(lib.tg_conv3x3_wino_fused_fwd(a, px // 4 - 1, b, None, c, py, n, cin, cout, h, w, 0, 2, None), 'x')
    refused(lib.tg_conv3x3_small_fwd(a, px - 1, b, None, None, 0, 1, c, 3 * h * w, n, cin, 3, h, w, 0, None), 'x')
    refused(lib.tg_conv3x3_small_fwd(a, px, b, None, None, 0, 1, c, 3 * h * w - 1, n, cin, 3, h, w, 0, None), 'y')
    refused(lib.tg_conv3x3_small_fwd_res(a, px, b, None, d, 3 * h * w - 4, c, 3 * h * w, n, cin, 3, h, w, 0, None), 'res')
    refused(lib.tg_conv3x3_fewin_fwd(a, 3 * h * w - 4, b, None, 0, c, py, n, 3, cout, h, w, None), 'x')
    refused(lib.tg_conv3x3_fewin_fwd(a, 3 * h * w, b, d, py - 4, c, py, n, 3, cout, h, w, None), 'mask')
    refused(lib.tg_conv3x3_fewin_fwd(a, 3 * h * w, b, None, 0, c, py - 4, n, 3, cout, h, w, None), 'y')
    refused(lib.tg_convt3x3s2_fwd(a, px - 1, b, None, c, 4 * py, n, cin, cout, h, w, 0, None), 'x')
    refused(lib.tg_convt3x3s2_fwd(a, px, b, None, c, 4 * py - 2, n, cin, cout, h, w, 0, None), 'y')
    for z_entry in (lambda xs, zs: lib.tg_convt3x3s2_z_fwd_form(a, xs, b, None, d, 3, c, zs, n, cin, cout, h, w, 1, 0, None),
                    lambda xs, zs: lib.tg_convt3x3s2_z_wino_fwd(a, xs, b, None, d, 3, c, zs, n, cin, cout, h, w, 1, 0, None)):
        refused(z_entry(px - 1, 32 * 4 * h * w), 'x')
        refused(z_entry(px, 27 * 4 * h * w - 2), 'z')            # the 9 cz planes it writes
    refused(lib.tg_convout_tail_form(a, 27 * h * w - 1, 3, None, None, 0, 1, c, 3 * h * w, None, n, h, w, -1, None), 'z')
    refused(lib.tg_convout_tail_form(a, 32 * h * w, 3, None, None, 0, 1, c, 3 * h * w - 1, None, n, h, w, -1, None), 'y')
    refused(lib.tg_conv3x3_f16_pack_input(a, 3 * h * w - 1, 3, b, 48 * h * w, 48, c, n, h, w, None), 'x1')
    refused(lib.tg_conv3x3_f16_pack_input(a, 3 * h * w, 3, b, 48 * h * w - 1, 48, c, n, h, w, None), 'x2')
    refused(lib.tg_flowup_warp_s2d_fwd(a, 8, 8, b, c, 48 * 8 * 8 - 1, None, n, 3, 8, 8, 4, 1, None), 'out')
    refused(lib.tg_space_to_depth(a, c, 3 * h * w - 1, n, 3, h, w, 2, None), 'y')
    assert lib.tg_convt3x3s2_f16_fwd(a, b, d, c, 64 * 4 * h * w - 2, n, 64, 64, h, w, 0, None) == E      # (as before)


def test_alignment_gates_that_were_missing(lib, host):
    """tg_convt3x3s2_z_wino_fwd checked neither the base nor the stride of z although it stores 16 / 8 bytes at even
    float offsets of an image: now the direct form's contract (TG_E_ARG).  tg_conv4x4s2_fwd / _dgrad let any pointer
    through to the 16-byte summing launch of the small-map forms: TG_E_ARG now.  The gates that existed are
    asserted next to them, so that the table in KERNELS.md is checked where no GPU is needed."""
    _, (a, b, c, d) = host
    n, cin, cout, h, w = 2, 64, 64, 6, 8
    zs = 32 * 4 * h * w
    A = -2
    for z, ns in ((c + 4, zs), (c, zs + 1), (c + 12, zs)):
        assert lib.tg_convt3x3s2_z_wino_fwd(a, cin * h * w, b, None, d, 3, z, ns, n, cin, cout, h, w, 1, 0, None) == A
        assert b'8-byte aligned' in lib.tg_last_error_string()
        assert lib.tg_convt3x3s2_z_fwd_form(a, cin * h * w, b, None, d, 3, z, ns, n, cin, cout, h, w, 1, 0, None) == A
    assert lib.tg_convt3x3s2_fwd(a, cin * h * w, b, None, c + 4, cout * 4 * h * w, n, cin, cout, h, w, 0, None) == A
    assert lib.tg_convt3x3s2_fwd(a, cin * h * w, b, None, c, cout * 4 * h * w + 1, n, cin, cout, h, w, 0, None) == A
    # conv4x4s2: (2, 64, 128, 16, 16) splits the input channels (it needs a workspace); (2, 64, 64, 2, 64) does not
    assert lib.tg_conv4x4s2_workspace_floats(2, 64, 128, 16, 16, 0) > 0 and lib.tg_conv4x4s2_workspace_floats(2, 64, 64, 2, 64, 0) == 0
    assert lib.tg_conv4x4s2_fwd(a, b, c + 4, d, 2, 64, 128, 16, 16, None) == A
    assert b'16-byte aligned' in lib.tg_last_error_string()
    assert lib.tg_conv4x4s2_fwd(a, b, c, d + 8, 2, 64, 128, 16, 16, None) == A
    assert lib.tg_conv4x4s2_fwd(a, b, c, None, 2, 64, 128, 16, 16, None) == A
    assert lib.tg_conv4x4s2_workspace_floats(2, 64, 128, 16, 16, 1) > 0
    assert lib.tg_conv4x4s2_dgrad(a, b, None, 0, c + 4, d, 2, 64, 128, 16, 16, None) == A
    assert lib.tg_conv4x4s2_dgrad(a, b, a + 8, 1, c, d, 2, 64, 128, 16, 16, None) == A
    # the forms without a scalar fallback: misplaced operands are TG_E_ARG / TG_E_SHAPE
    px, py = 3 * h * w, cout * h * w
    assert lib.tg_conv3x3_fewin_fwd(a + 4, px, b, None, 0, c, py, n, 3, cout, h, w, None) == A
    assert lib.tg_conv3x3_fewin_fwd(a, px, b, d + 8, py, c, py, n, 3, cout, h, w, None) == A
    assert lib.tg_conv3x3_fewin_fwd(a, px, b, None, 0, c, py + 1, n, 3, cout, h, w, None) == A
    assert lib.tg_conv3x3_fewin_fwd(a, 3 * 5 * 7, b, None, 0, c, cout * 5 * 7, n, 3, cout, 5, 7, None) == A
    assert lib.tg_conv3x3_small_fwd_res(a, cin * h * w, b, None, d + 4, 3 * h * w, c, 3 * h * w, n, cin, 3, h, w, 0, None) == A
    assert lib.tg_conv3x3_small_fwd_res(a, cin * h * w, b, None, d, 3 * h * w, c + 8, 3 * h * w, n, cin, 3, h, w, 0, None) == A
    assert lib.tg_convout_tail_form(a, 32 * h * w, 3, None, None, 0, 1, c + 4, 3 * h * w, None, n, h, w, 1, None) == -1
    assert lib.tg_convout_tail_form(a, 32 * 35, 3, None, None, 0, 1, c, 3 * 35, None, n, 5, 7, 1, None) == -1
    assert lib.tg_conv3x3_f16_pack_input(a, px, 3, None, 0, 0, c + 8, n, h, w, None) == A
