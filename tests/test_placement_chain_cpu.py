"""CPU: what tests/test_hip_placement_chain.py stands on, without a GPU (the manner of tests/test_placement_bwd_cpu.py).

1. Through the C ABI with host addresses: the refusals of the one-launch bodies that are decided before any device
   query -- TG_REQUIRE_LAYER_NSTRIDE for x, x2, res, relu_mask and y of every layer of tg_conv3x3_wino_chain and
   tg_conv3x3_chain ("layer %d: <operand>_nstride", TG_E_SHAPE).  (The alignment refusals of tg_conv3x3_wino_resident
   sit behind conv3x3_wino_resident_ok, a device query: the GPU file asserts them.)
2. The host-side form choice of conv3x3_wino_chain_launch (vec_ok) and the per-layer, per-image store form of the two
   conv3x3_rowchain_kernel instances are restated in Python, and the GPU case tables crossed with the placements are
   checked to reach both values of each, for every reason a launch can leave the vector form.
3. ops.WinoChain / WinoResident / RowChain refuse a float64 and a channels-last tensor before they take a pointer.
4. The two additions to tests/placement.py: an alignment of its own for one operand, and a destination that starts as
   zeros."""
import ctypes

import pytest
import torch

from tecogan_pytorch_amd._lib import TG_E_SHAPE
from tests import test_hip_placement_chain as G
from tests.placement import Arena, GUARD
from tests.test_hip_placement import al

N = G.N


@pytest.fixture(scope='module')
def lib():
    from tecogan_pytorch_amd import _lib
    return _lib.lib()


@pytest.fixture(scope='module')
def host():
    buf = (ctypes.c_char * (12 << 16))()
    a = (ctypes.addressof(buf) + 63) & ~63
    return buf, [a + (i << 16) for i in range(11)]


# ======================================================================================================================
# 1. the contract through the C ABI (host addresses; nothing is launched)
# ======================================================================================================================
def refused(lib, rc, layer, what):
    msg = lib.tg_last_error_string().decode()
    assert rc == TG_E_SHAPE and f'layer {layer}: {what}_nstride' in msg and 'one image' in msg, (rc, msg)


def test_wino_chain_batch_strides_smaller_than_an_image_are_refused(lib, host):
    """conv3x3_wino_chain_launch copied the four strides of every layer into the kernel arguments unchecked: with n > 1 a
    stride below one image computed on overlapping images and returned TG_OK."""
    from tecogan_pytorch_amd import _lib as L
    _, (x, x2, u, b, A, B, flags, *_) = host
    h, w, hw = 4, 6, 24

    def layers(**short):
        arr = (L.WinoLayer * 3)()
        full = [dict(x=x, x2=x2, res=None, y=A, xs=3 * hw, x2s=48 * hw, rs=0, ys=64 * hw, c1=3, cin=51, act=1),
                dict(x=A, x2=None, res=None, y=B, xs=64 * hw, x2s=0, rs=0, ys=64 * hw, c1=64, cin=64, act=1),
                dict(x=B, x2=None, res=A, y=A, xs=64 * hw, x2s=0, rs=64 * hw, ys=64 * hw, c1=64, cin=64, act=0)]
        for i, (a, d) in enumerate(zip(arr, full)):
            a.x, a.x2, a.u_packed, a.bias, a.res, a.y = d['x'], d['x2'], u, b, d['res'], d['y']
            a.x_nstride, a.x2_nstride, a.res_nstride, a.y_nstride = d['xs'], d['x2s'], d['rs'], d['ys']
            a.c1, a.cin, a.act = d['c1'], d['cin'], d['act']
            for k, field in (('x', 'x_nstride'), ('x2', 'x2_nstride'), ('res', 'res_nstride'), ('y', 'y_nstride')):
                if short.get('layer') == i and short.get('field') == k:
                    setattr(a, field, getattr(a, field) - 1)
        return arr
    for layer, field in ((0, 'x'), (0, 'x2'), (0, 'y'), (1, 'x'), (1, 'y'), (2, 'x'), (2, 'res'), (2, 'y')):
        refused(lib, lib.tg_conv3x3_wino_chain(layers(layer=layer, field=field), 3, 2, 64, h, w, flags, 1, None), layer, field)
    # the checks that were there come first and keep their codes
    assert lib.tg_conv3x3_wino_chain(layers(layer=0, field='x'), 3, 2, 64, h, w, flags, 0, None) == -2      # epoch 0
    assert lib.tg_conv3x3_wino_chain(layers(layer=0, field='x'), 3, 2, 65, h, w, flags, 1, None) == -1      # cout > 64
    assert b'nstride' not in lib.tg_last_error_string()


def test_row_chain_batch_strides_smaller_than_an_image_are_refused(lib, host):
    """tg_conv3x3_chain had no stride check either; the checks stand in front of tg_conv3x3_chain_supported (a device
    query), so they are reached here.  The last layer of the backward pattern has cout = 48: its y is 48 planes."""
    from tecogan_pytorch_amd import _lib as L
    _, (g, m1, m0, wp, d1, d0, dt, flags, err, *_) = host
    h, w, hw = 4, 6, 24

    def layers(layer=None, field=None):
        arr = (L.ChainLayer * 3)()
        full = [dict(x=g, res=None, mask=m1, y=d1, cout=64), dict(x=d1, res=g, mask=m0, y=d0, cout=64),
                dict(x=d0, res=None, mask=None, y=dt, cout=48)]
        for i, (a, d) in enumerate(zip(arr, full)):
            a.x, a.w_packed, a.res, a.relu_mask, a.y = d['x'], wp, d['res'], d['mask'], d['y']
            a.x_nstride, a.res_nstride, a.mask_nstride, a.y_nstride = 64 * hw, 64 * hw, 64 * hw, d['cout'] * hw
            a.c1, a.cin, a.cout, a.act = 64, 64, d['cout'], 0
            if layer == i:
                setattr(a, f'{field}_nstride', getattr(a, f'{field}_nstride') - 1)
        return arr
    for layer, field in ((0, 'x'), (0, 'mask'), (0, 'y'), (1, 'x'), (1, 'res'), (1, 'mask'), (1, 'y'), (2, 'x'), (2, 'y')):
        refused(lib, lib.tg_conv3x3_chain(layers(layer, field), 3, 2, h, w, 16, flags, err, 1, 1 << 21, None), layer, field)
    # a second source
    arr = layers()
    arr[0].x2, arr[0].c1, arr[0].cin, arr[0].x_nstride, arr[0].x2_nstride = m0, 3, 51, 3 * hw, 48 * hw - 1
    refused(lib, lib.tg_conv3x3_chain(arr, 3, 2, h, w, 16, flags, err, 1, 1 << 21, None), 0, 'x2')
    arr[0].x_nstride, arr[0].x2_nstride = 3 * hw - 1, 48 * hw
    refused(lib, lib.tg_conv3x3_chain(arr, 3, 2, h, w, 16, flags, err, 1, 1 << 21, None), 0, 'x')
    assert lib.tg_conv3x3_chain(layers(0, 'x'), 3, 2, h, w, 16, flags, err, 0, 1 << 21, None) == -2        # epoch 0 first


# ======================================================================================================================
# 2. the form choices, restated
# ======================================================================================================================
def wino_chain_vec_ok(info, spec, h, w):
    """conv3x3_wino_chain_launch: ONE vec_ok for the launch -- w and h w even, y and res of EVERY layer 8-byte aligned
    with even strides.  Returns 'vector', or why not."""
    if w % 2 or (h * w) % 2:
        return 'by shape'
    names = {d['y'] for d in spec} | {d['res'] for d in spec if d['res']}
    bad_ptr = [k for k in names if info[k][0] % 2]
    bad_ns = [k for k in names if info[k][1] % 2]
    if not bad_ptr and not bad_ns:
        return 'vector'
    if len(bad_ptr) + len(bad_ns) == 1 and len(names) > 1:
        return 'by one tensor'
    return 'by stride' if bad_ns and not bad_ptr else 'by pointer'


def test_wino_chain_cases_reach_both_epilogues_for_every_reason(lib):
    reached = {}
    for h, w, cin0, c1 in G.WINO_CHAIN_CASES:
        for pattern in G.PATTERNS:
            case = G.wino_chain_case(lib, h, w, cin0, c1, pattern)
            spec = G.wino_spec(pattern, bool(c1))
            for tag, info in case.infos():
                assert case.expect(info) == 0                       # every placement is launched
                why = wino_chain_vec_ok(info, spec, h, w)
                reached.setdefault((h, w), set()).add(why)
                # the restated rule agrees with the helper of the single-layer file on every tensor
                assert (why == 'vector') == (w % 2 == 0 and h * w % 2 == 0 and all(
                    al(info, d['y'], 2) and (not d['res'] or al(info, d['res'], 2)) for d in spec))
                if tag.split('@')[0] in ('x', 'x2', 'flags'):       # the sources and the flags never decide
                    assert why == wino_chain_vec_ok(dict(case.infos())['P0'], spec, h, w)
            assert [t for t, _ in case.infos()].count('P0') == 1
    assert reached[(4, 64)] == {'vector', 'by one tensor', 'by pointer', 'by stride'}
    assert reached[(4, 34)] == reached[(4, 64)] and reached[(3, 33)] == {'by shape'}
    # P2 and P4 keep the float2 epilogue, P1 and P3 lose it; P5 (3 h w floats more per image) keeps it where 3 h w is even
    case = G.wino_chain_case(lib, 4, 64, 51, 3, 'own')
    by_tag = dict(case.infos())
    spec = G.wino_spec('own', True)
    assert [wino_chain_vec_ok(by_tag[f't1@{p}'], spec, 4, 64) for p in ('P1', 'P2', 'P3', 'P4', 'P5')] == \
        ['by one tensor', 'vector', 'by one tensor', 'vector', 'vector']
    assert wino_chain_vec_ok(by_tag['all@P1'], spec, 4, 64) == 'by pointer' and wino_chain_vec_ok(by_tag['all@P3'], spec, 4, 64) == 'by stride'
    # a tensor that one layer writes and another reads is one operand: the ping-pong pattern has two of them
    srnet = G.wino_chain_case(lib, 4, 64, 51, 3, 'srnet')
    assert sorted(o.name for o in srnet.operands if getattr(o, 'inout', False)) == ['A', 'B']
    assert [o.shape for o in srnet.operands if o.name == 'flags'] == [(lib.tg_conv3x3_wino_chain_flag_ints(3, N, 4, 64),)]
    one_k_stage = [c for c in G.WINO_CHAIN_CASES if c[2] <= 16]
    assert one_k_stage and all(c[3] is None for c in one_k_stage)


def row_chain_store_form(info_y, h, w, per, image):
    """conv3x3_rowchain_kernel<8> (per = 2) / <4> (per = 4), per layer and image:
    vec && (yp & 15) == 0 && hw % 4 == 0 && y_ns % 4 == 0 with vec = w % per == 0 and yp = y + image * y_ns."""
    off, ns = info_y
    return w % per == 0 and (off + image * ns) % 4 == 0 and (h * w) % 4 == 0 and ns % 4 == 0


@pytest.mark.parametrize('direction', ['fwd', 'bwd'])
def test_row_chain_large_maps_reach_both_store_forms_per_image(lib, direction):
    """Which map tg_conv3x3_chain_supported sends to the 32 x 32 x 2 kernels is a device query; whatever it answers, the
    map is n = 2, w = 32, and at the placements the larger maps run at the store form goes: P0 vector for both images,
    all@P1 neither (by pointer), all@P3 neither (y_nstride % 4, which would leave image 1 at 4 bytes), all@P4 both."""
    for h in (36, 65, 130):                      # (any h: w = 32 carries the rule; h w % 4 == 0 with it)
        for pattern in G.PATTERNS:
            case = G.row_chain_case(lib, h, 32, direction, pattern, parts=2, only=G.ROW_CHAIN_LARGE_TAGS)
            tags = [t for t, _ in case.infos()]
            assert tags == ['P0', 'all@P1', 'all@P3', 'all@P4']
            dests = [o.name for o in case.operands if o.kind == 'out' and o.name != 'flags']
            for per in (2, 4):
                got = {t: [[row_chain_store_form(info[k], h, 32, per, b) for b in range(N)] for k in dests]
                       for t, info in case.infos()}
                assert all(f == [True, True] for f in got['P0']) and all(f == [False, False] for f in got['all@P1'])
                assert all(f == [False, False] for f in got['all@P3']) and all(f == [True, True] for f in got['all@P4'])
    # the small tables: every destination is a strided operand of its own, the last backward layer 48 planes
    case = G.row_chain_case(lib, 5, 40, 'bwd', 'own', parts=4)
    shapes = {o.name: o.shape for o in case.operands}
    assert shapes['d_tran'] == (N, 48, 5, 40) and shapes['dz0'] == (N, 64, 5, 40)
    assert shapes['flags'] == (lib.tg_conv3x3_chain_flag_ints(3, N, 5, 40) + 16,)
    assert any(w % 4 == 0 for _, w in G.ROW_CHAIN_CASES) and any(w % 2 for _, w in G.ROW_CHAIN_CASES)
    assert any((w + 31) // 32 > 1 for _, w in G.ROW_CHAIN_CASES)


def test_resident_and_body_cases_move_bases_only(lib):
    for h, w in G.WINO_RES_CASES:
        assert h % 2 == 0 and w % 2 == 0
        for pattern in G.PATTERNS:
            for tail in (False, True):
                case = G.wino_res_case(lib, h, w, pattern, tail)
                tags = [t for t, _ in case.infos()]
                assert all(t == 'P0' or t.split('@')[1] in ('P1', 'P2') for t in tags)
                last = 't2' if pattern == 'own' else 'A'
                moved = {t.split('@')[0] for t in tags} - {'P0', 'all'}
                assert moved == {'x', 'x2', last, 'ws'} | ({'ct_y'} if tail else set())
                by_tag = dict(case.infos())
                # the workspace moves alone (refused: 256-byte alignment) and stays put in the all@ placements
                assert by_tag['ws@P1']['ws'][0] == 1 and by_tag['all@P2']['ws'][0] == 0
                want = {'P0': 0, f'{last}@P1': -2, f'{last}@P2': 0, 'x@P1': 0, 'x2@P2': 0, 'ws@P1': -2, 'ws@P2': -2, 'all@P1': -2,
                        'all@P2': -2 if tail else 0}
                if tail:
                    want.update({'ct_y@P1': -2, 'ct_y@P2': -2})
                assert {t: case.expect(by_tag[t]) for t in want} == want
                ws = [o for o in case.operands if o.name == 'ws'][0]
                assert ws.shape == (lib.tg_conv3x3_wino_resident_ws_bytes(h, w) // 4,) and ws.align == 64 and ws.zero
    assert {(-(-h // 8)) * (-(-w // 24)) for h, w in G.WINO_RES_CASES} == {1, 4}
    for h, w in G.BODY_CASES:
        for direction in ('fwd', 'bwd'):
            case = G.body_case(lib, h, w, direction, parts=4, acts=torch.zeros(3 * N, 64, h, w))
            moved = {t.split('@')[0] for t, _ in case.infos()} - {'P0', 'all'}
            assert moved == ({'lr', 'tran', 'acts', 'flags'} if direction == 'fwd' else {'acts', 'dz', 'd_tran', 'flags'})
            assert all(t == 'P0' or t.split('@')[1] in ('P1', 'P2') for t, _ in case.infos())


# ======================================================================================================================
# 3. the wrappers
# ======================================================================================================================
def test_chain_wrappers_refuse_foreign_dtypes_and_layouts():
    """ops.WinoChain / WinoResident / RowChain took data_ptr() and stride(0) of whatever they were given.  dtype and
    layout are checked before the device, so the refusals show here; a batch stride of its own is still allowed."""
    import tecogan_pytorch_amd.ops as ops
    from tecogan_pytorch_amd._lib import TecoganHipError
    good = torch.zeros(2, 64, 4, 6)
    f64 = torch.zeros(2, 64, 4, 6, dtype=torch.float64)
    nhwc = torch.zeros(2, 64, 4, 6).contiguous(memory_format=torch.channels_last)
    wide = torch.zeros(2, 67, 4, 6)[:, :64]                     # a channel slice: inner dimensions contiguous
    assert ops._chk_batched.__doc__ and wide.stride(0) == 67 * 24 and not wide.is_contiguous()
    u = torch.zeros(16)
    for cls, build in (('WinoChain', lambda x, y: ops.WinoChain([dict(x=x, u=u, cin=64, y=y)], 2, 64, 4, 6)),
                       ('WinoResident', lambda x, y: ops.WinoResident([dict(x=x[:1], u=u, cin=64, y=y[:1])], 64, 4, 6)),
                       ('RowChain', lambda x, y: ops.RowChain([dict(x=x, w=torch.zeros(64, 64, 3, 3), y=y)], 2, 4, 6))):
        for bad, word in ((f64, 'float32'), (nhwc, 'contiguous')):
            with pytest.raises(TecoganHipError, match=word):
                build(bad, good)
            with pytest.raises(TecoganHipError, match=word):
                build(good, bad)
        with pytest.raises(TecoganHipError, match='CUDA/HIP tensor'):      # the layout passes, the device does not
            build(wide, good)
    with pytest.raises(TecoganHipError, match='contiguous'):
        ops._chk_batched(torch.zeros(2, 64, 4, 6)[::2].expand(2, 64, 4, 6), 'x')     # images that overlap


# ======================================================================================================================
# 4. tests/placement.py: an alignment of its own, a destination that starts as zeros
# ======================================================================================================================
def test_arena_alignment_and_zeroed_destinations():
    a = Arena('cpu', margin_floats=300, slots=3, align_floats=64)
    x = a.place(torch.arange(24, dtype=torch.float32).reshape(2, 3, 4), offset_floats=1, name='x')
    ws = a.out((200,), name='ws', align_floats=64, zero=True)
    y = a.out((2, 5), offset_floats=2, nstride=7, name='y', zero=True)
    assert ws.data_ptr() % 256 == 0 and x.data_ptr() % 64 == 4 and y.data_ptr() % 64 == 8
    assert torch.equal(x, torch.arange(24, dtype=torch.float32).reshape(2, 3, 4))
    assert int(ws.view(torch.int32).abs().sum()) == 0 and int(y.view(torch.int32).abs().sum()) == 0
    a.check(outputs_untouched=True)                          # zeros are what a refusal must leave behind
    a.finite(ws)
    ws[-64:] = 1.0
    y[:] = 2.0
    a.check()
    with pytest.raises(AssertionError, match='outside the destination'):
        a.check(outputs_untouched=True)
    a.words[y._arena_op['base'] + 5] = 0                     # the gap between the images of y keeps the guard pattern
    with pytest.raises(AssertionError, match='gap behind image 0'):
        a.check()
    # the default is what it was: 64-byte boundaries, one allocation of the same size
    d = Arena('cpu', margin_floats=300, slots=3)
    assert d.total == 3 * (3 * 300 + 64) + 16 and d.words.storage_offset() == 0
    with pytest.raises(AssertionError, match='alignment'):
        d.out((8,), align_floats=64)
    assert (GUARD & 0xFF) == 0
