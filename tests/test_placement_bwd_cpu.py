"""CPU: what tests/test_hip_placement_bwd.py stands on, without a GPU (the pattern of parts 2 and 3 of
tests/test_placement_cpu.py).

2. The host-side choices of the backward launchers that depend on shape or placement are restated here in Python, next
   to the names of the code they restate, and the GPU case tables crossed with the placements are checked to reach
   every value of each: every kernel form with the vector staging AND with the element-wise staging, the latter by
   shape, by pointer, by stride, by one segment of a list and by lstride; both sides of fuse_a and fuse_b.
3. Through the C ABI with host addresses (every check comes before any launch): the refusals this change adds, the
   gates that existed, and each workspace query against the restated split rule for every case of the tables."""
import ctypes

import pytest

from tests import test_hip_placement_bwd as G
from tests.placement import Arena

N = G.N


def cdiv(a, b):
    return (a + b - 1) // b


@pytest.fixture(scope='module')
def lib():
    from tecogan_pytorch_amd import _lib
    return _lib.lib()


def al4(op_info):
    return op_info[0] % 4 == 0 and op_info[1] % 4 == 0


# ======================================================================================================================
# 2. tg_wgrad_mfma.hip, restated
# ======================================================================================================================
def wgrad_geo(h, w):
    """wgrad_geo: 0 = 2 x 32, 1 = 4 x 16, 2 = 8 x 8."""
    return 2 if w <= 8 and h > 2 else (1 if w <= 16 and h > 2 else 0)


def wgrad_kmode(ca, cb, cb_total):
    """wgrad_kmode."""
    return (1 if ca <= 32 else 0) | (2 if cb <= 32 and cb_total <= 64 else 0)


def wgrad_tile(geo):
    """wgrad_tile: (rows, columns) of a pixel tile; geo 3 = the stride-2 form."""
    return {0: (2, 32), 1: (4, 16), 2: (8, 8), 3: (1, 32)}[geo]


SC_MAXBLK, SC_TR, SC_TW = 768, 4, 32


def wgrad_nsplit(n, h, w, ca, cb, geo=0):
    """wgrad_nsplit: persistent blocks of the small-ca kernel, else the K split of the MFMA kernel."""
    if ca <= 4 and geo != 3:
        nt, per_b = n * cdiv(h, SC_TR) * cdiv(w, SC_TW), SC_MAXBLK // cdiv(cb, 64)
        nb = nt if nt < per_b else (per_b if per_b > 0 else 1)
        lim = 256 // cdiv(cb, 64)
        if nb > lim and nb * 3 > nt:
            nb = nt // 3 if nt // 3 > lim else lim
        return nb if nb > 0 else 1
    r, tw = wgrad_tile(geo)
    return max(1, min(512 // (cdiv(ca, 64) * cdiv(cb, 64)), n * cdiv(h, r) * cdiv(w, tw), 256))


def wgrad_form(ca, cb, cb_total, h, w, phased=False, stride2=False):
    """The dispatch of wgrad_launch: which kernel runs (before the staging form is chosen)."""
    if ca <= 4 and not phased and not stride2:
        return f'smallca<{min(ca, 4)}>'
    if cb <= 4 and not phased and not stride2:
        return f'swapped smallca<{min(cb, 4)}>'
    geo = 3 if stride2 else (0 if phased else wgrad_geo(h, w))
    if geo:
        return f'geo{geo}'
    km = 0 if phased else wgrad_kmode(ca, cb, cb_total)
    return 'phased' if phased else {0: 'std', 1: 'ks2 (a)', 2: 'ks2 (b)', 3: 'ks4'}[km]


def staging(w, p_infos, q_infos, lstride=0):
    """wgrad_vec_ok (and the same rule in launch_smallca): 'vector', or why the launch is element-wise."""
    if w % 4:
        return 'by shape'
    if lstride % 4:
        return 'by lstride'
    infos = list(p_infos) + list(q_infos)
    if any(i[1] % 4 for i in infos):
        return 'by stride'
    bad = [i for i in infos if i[0] % 4]
    if not bad:
        return 'vector'
    return 'by one segment' if len(bad) == 1 and len(infos) > 2 else 'by pointer'


def wgrad_need(nimg, ca, cb, cb_total, h, w, form, bias_fused):
    """The floats a launch of wgrad_launch writes into its workspace: partial sums [split][ks][ca][cb_total][9] (the
    exchanged small-ca form: [block][cb][ca][9]) and, behind them, the bias partials [split][ca] of fuse_a."""
    if form.startswith('smallca'):
        return wgrad_nsplit(nimg, h, w, ca, cb_total) * ca * cb_total * 9
    if form.startswith('swapped'):
        return wgrad_nsplit(nimg, h, w, cb, ca) * cb * ca * 9
    geo = {'geo1': 1, 'geo2': 2}.get(form, 0)
    ns = wgrad_nsplit(nimg, h, w, ca, cb_total, geo)
    ks = {'ks2 (a)': 2, 'ks2 (b)': 2, 'ks4': 4}.get(form, 1)
    return ns * ks * ca * cb_total * 9 + (ns * ca if bias_fused else 0)


def seg_infos(info, prefix):
    return [v for k, v in sorted(info.items()) if k.startswith(prefix) and k[len(prefix):].isdigit()]


def test_wgrad_cases_reach_every_form_with_both_stagings_and_every_reason(lib):
    reached, fuse_a = {}, set()
    runs = [(e, s, r) for r in G.WGRAD_CASES for e, s in G.WGRAD_ENTRIES] + [(e, s, G.WGRAD_CASES[i]) for e, s, i in G.WGRAD_EXTRA]
    for entry, nseg, (ca, cb, cbt, off, h, w) in runs:
        form = wgrad_form(ca, cb, cbt, h, w)
        case = G.wgrad_case(lib, entry, nseg, ca, cb, cbt, off, h, w)
        wsf = dict((o.name, o.shape) for o in case.operands)['workspace'][0]
        assert wsf == lib.tg_wgrad3x3_workspace_floats(N * nseg, ca, cbt, h, w)          # exactly the query, never more
        for tag, info in case.infos():
            if case.expect(info) != 0:
                assert entry == 'bias' and tag.split('@')[0] in ('p_list', 'all')          # the packed-p refusal
                continue
            st = staging(w, seg_infos(info, 'p'), seg_infos(info, 'q'))
            reached.setdefault(form, set()).add(st)
            fused = entry == 'bias' and st == 'vector' and 'smallca' not in form            # fuse_a
            if entry == 'bias':
                fuse_a.add((form, fused))
            assert wsf >= wgrad_need(N * nseg, ca, cb, cbt, h, w, form, fused), (form, tag)
    assert set(reached) == {'std', 'ks2 (a)', 'ks2 (b)', 'ks4', 'geo1', 'geo2', 'smallca<3>', 'smallca<2>', 'swapped smallca<3>'}
    for form, seen in reached.items():
        # the vector staging and, on the same (aligned) shape, the element-wise one by a pointer, by a stride and by
        # one segment of three
        assert {'vector', 'by pointer', 'by stride', 'by one segment'} <= seen, (form, seen)
    assert 'by shape' in reached['std']
    # the bias gradient rides on the launch (fuse_a) and runs behind it, on every MFMA form; never on the small-ca forms
    for form in ('std', 'ks2 (a)', 'ks2 (b)', 'ks4', 'geo1', 'geo2'):
        assert {(form, True), (form, False)} <= fuse_a, form
    assert {f for f, on in fuse_a if 'smallca' in f} == {'smallca<3>', 'smallca<2>', 'swapped smallca<3>'}
    assert not any(on for f, on in fuse_a if 'smallca' in f)
    # the rows the issue names
    assert wgrad_geo(3, 40) == 0 and wgrad_geo(6, 16) == 1 and wgrad_geo(6, 8) == 2 and wgrad_geo(2, 8) == 0
    assert [wgrad_kmode(*r[:3]) for r in G.WGRAD_CASES[4:7]] == [1, 2, 3]
    assert any(r[3] > 0 and r[1] < r[2] for r in G.WGRAD_CASES) and any(cdiv(r[0], 64) * cdiv(r[1], 64) == 4 for r in G.WGRAD_CASES)


def test_phased_convt_and_body_cases_reach_both_stagings_and_both_sides_of_fuse_b(lib):
    seen = set()
    for ca, cb, cphase, h, w, t0, t1, nseg in G.PHASED_CASES:
        assert cphase % 64 == 0 and cb == 4 * cphase and wgrad_form(ca, cb, cb, h, w, phased=True) == 'phased'
        case = G.wgrad_case(lib, 'phased', nseg, ca, cb, cb, 0, h, w, phased=(cphase, t0, t1))
        for tag, info in case.infos():
            seen.add(staging(w, seg_infos(info, 'p'), seg_infos(info, 'q')))
        # the phased launch uses the 2 x 32 tile whatever the map: the query sizes for the larger of the two counts
        assert lib.tg_wgrad3x3_workspace_floats(N * nseg, ca, cb, h, w) >= wgrad_nsplit(N * nseg, h, w, ca, cb, 0) * ca * cb * 9
    assert {'vector', 'by pointer', 'by stride', 'by one segment'} <= seen
    assert {(c[5], c[6]) for c in G.PHASED_CASES} == {(G.TAPS_12, G.TAPS_01), (G.TAPS_1, G.TAPS_01)}     # train_graph.py's two
    fuse_b = set()
    for ci, co, h, w in G.CONVT_W_CASES:
        assert wgrad_form(ci, co, co, h, w, stride2=True) == 'geo3'
        for nseg in G.CONVT_W_SEGS:
            case = G.convt_wgrad_case(lib, nseg, ci, co, h, w, True)
            wsf = lib.tg_wgrad3x3_convt_workspace_floats(N * nseg, ci, co, h, w)
            ns = wgrad_nsplit(N * nseg, h, w, ci, co, 3)
            assert wsf >= ns * ci * co * 9 + ns * co                                      # + the bias partials of fuse_b
            for tag, info in case.infos():
                st = staging(w, seg_infos(info, 'x'), seg_infos(info, 'dz'))
                fuse_b.add((st, st == 'vector' and cdiv(co, 64) == 1))                    # fuse_b = bias && vec && nbb == 1
    assert {('vector', True), ('vector', False), ('by pointer', False), ('by one segment', False)} <= fuse_b
    body = set()
    for c, nl, frames, h, w in G.BODY_CASES:
        case = G.body_case(lib, 'body_bias', c, nl, frames, h, w)
        ntiles = frames * N * cdiv(h, 2) * cdiv(w, 32)
        ns = max(1, min(1280 // (nl * cdiv(c, 64) ** 2), ntiles, 256))                    # body_nsplit
        assert lib.tg_wgrad3x3_body_workspace_floats(frames, N, nl, c, h, w) >= nl * ns * c * c * 9 + nl * ns * c
        for tag, info in case.infos():
            blocks = seg_infos(info, 'dz') + seg_infos(info, 'act')
            ls = blocks[0][1]
            assert all(b[1] == ls for b in blocks)                                       # one layer_stride per launch
            # (the per-image stride inside a layer is packed: c h w; wgrad_vec_ok sees lstride and the bases)
            body.add(staging(w, [(b[0], 0) for b in blocks], [], lstride=ls))
    assert body == {'vector', 'by shape', 'by pointer', 'by one segment', 'by lstride'}, body
    packed = N * 64 * 4 * 8
    dz = [o for o in G.body_case(lib, 'body', 64, 3, 2, 4, 8).operands if o.name == 'dz0'][0]
    assert [dz.resolve(p)[1] for p in ('P0', 'P3', 'P4')] == [packed, packed + 1, packed + 8]


def test_every_segment_is_an_operand_and_a_list_moves_as_one(lib):
    case = G.wgrad_case(lib, 'multi', 3, 64, 64, 64, 0, 6, 8)
    tags = [t for t, _ in case.placements()]
    assert tags == ['p0@P1', 'p0@P2', 'p1@P1', 'p1@P2', 'p2@P1', 'p2@P2', 'q0@P1', 'q0@P2', 'q1@P1', 'q1@P2', 'q2@P1', 'q2@P2',
                    'grad@P1', 'grad@P2', 'workspace@P1', 'workspace@P2', 'p_list@P3', 'p_list@P4', 'q_list@P3', 'q_list@P4',
                    'all@P1', 'all@P2', 'all@P3', 'all@P4']
    by_tag = dict(case.infos())
    assert [by_tag['p_list@P3'][k][1] for k in ('p0', 'p1', 'p2', 'q0')] == [3073, 3073, 3073, 3072]
    assert by_tag['p1@P1']['p1'] == (1, 3072) and by_tag['p1@P1']['p0'] == (0, 3072)
    # Arena.inout: the column slice is writable and starts as the guard pattern, the other columns are inputs
    import torch
    a = Arena('cpu', margin_floats=256, slots=1)
    cols = torch.zeros(1, 5, 1, 1, dtype=torch.bool)
    cols[:, 1:3] = True
    g0 = torch.arange(2 * 5 * 9, dtype=torch.float32).reshape(2, 5, 3, 3)
    v = a.inout(g0, cols, True, name='grad')
    a.check(outputs_untouched=True)
    with pytest.raises(AssertionError, match='never written'):
        a.finite(v)
    v[:, 1:3] = 1.0
    a.check()
    a.finite(v)
    v[0, 0, 0, 0] = -1.0                                   # a foreign column
    with pytest.raises(AssertionError, match='nearest operand: grad'):
        a.check()


# ======================================================================================================================
# 3. the contract through the C ABI (host addresses; nothing is launched)
# ======================================================================================================================
@pytest.fixture(scope='module')
def host():
    buf = (ctypes.c_char * (9 << 16))()
    a = (ctypes.addressof(buf) + 63) & ~63
    return buf, [a + (i << 16) for i in range(8)]


def arr(*addrs):
    return (ctypes.c_void_p * len(addrs))(*addrs)


def test_wgrad_batch_strides_smaller_than_an_image_are_refused(lib, host):
    """wgrad_launch had no TG_REQUIRE_NSTRIDE: a p_nstride / q_nstride below one image computed on overlapping images
    and returned TG_OK.  Every entry that reaches it now returns TG_E_SHAPE and says which stride; n_per_seg = 1 never
    looks at it.  tg_bias_grad_body refuses layers that overlap."""
    _, (a, b, c, d, e, f, g, h_) = host
    ca, cb, h, w = 8, 16, 6, 8
    pp, pq = ca * h * w, cb * h * w

    def refused(rc, what):
        msg = lib.tg_last_error_string().decode()
        assert rc == -1 and f'{what}_nstride' in msg and 'one image' in msg, (rc, msg)
    refused(lib.tg_wgrad3x3(a, pp - 1, b, pq, c, d, 2, ca, cb, cb, 0, h, w, 0, None), 'p')
    refused(lib.tg_wgrad3x3(a, pp, b, pq - 1, c, d, 2, ca, cb, cb, 0, h, w, 0, None), 'q')
    refused(lib.tg_wgrad3x3_multi(arr(a, e), arr(b, f), 2, pp - 1, pq, c, d, 2, ca, cb, cb, 0, h, w, 0, None), 'p')
    refused(lib.tg_wgrad3x3_multi(arr(a, e), arr(b, f), 2, pp, pq - 1, c, d, 2, ca, cb, cb, 0, h, w, 0, None), 'q')
    refused(lib.tg_wgrad3x3_multi_bias(arr(a, e), arr(b, f), 2, pp, pq - 1, c, g, d, 2, ca, cb, cb, 0, h, w, 0, None), 'q')
    refused(lib.tg_wgrad3x3_multi_phased(arr(a), arr(b), 1, 64 * h * w, 256 * h * w - 1, c, d, 2, 64, 256, h, w, 0, 64, 2, 1, None), 'q')
    refused(lib.tg_wgrad3x3_multi_phased(arr(a), arr(b), 1, 64 * h * w - 1, 256 * h * w, c, d, 2, 64, 256, h, w, 0, 64, 2, 1, None), 'p')
    # the small-ca and exchanged forms sit behind the same check
    refused(lib.tg_wgrad3x3(a, 3 * h * w - 1, b, pq, c, d, 2, 3, cb, cb, 0, h, w, 0, None), 'p')
    refused(lib.tg_wgrad3x3(a, pp, b, 3 * h * w - 1, c, d, 2, ca, 3, 3, 0, h, w, 0, None), 'q')
    refused(lib.tg_wgrad3x3_multi_bias(arr(a, e), arr(b, f), 2, pp - 1, pq, c, g, d, 2, ca, cb, cb, 0, h, w, 0, None), 'p')
    # the bias gradient of tg_wgrad3x3_multi_bias reads p packed (its stand-alone reduction takes no stride); the gate
    # comes behind the shared checks (ca = 0: TG_E_SHAPE first)
    assert lib.tg_wgrad3x3_multi_bias(arr(a, e), arr(b, f), 2, pp + 8, pq, c, g, d, 2, 0, cb, cb, 0, h, w, 0, None) == -1
    for ns in (pp + 1, pp + 8):
        assert lib.tg_wgrad3x3_multi_bias(arr(a, e), arr(b, f), 2, ns, pq, c, g, d, 2, ca, cb, cb, 0, h, w, 0, None) == -2
        assert b'packed p' in lib.tg_last_error_string()
    # layered: layer_stride below one layer (as before), and the same for tg_bias_grad_body
    layer = 2 * 64 * h * w
    assert lib.tg_wgrad3x3_body(arr(a), arr(b), 1, layer - 1, 3, arr(c, d, e), f, 2, 64, h, w, 0, None) == -1
    assert lib.tg_wgrad3x3_body_bias(arr(a), arr(b), 1, layer - 1, 3, arr(c, d, e), arr(g, g, g), f, 2, 64, h, w, 0, None) == -1
    assert lib.tg_bias_grad_body(arr(a), 1, layer - 1, 3, arr(c, d, e), 2, 64, h * w, None) == -1
    assert b'layer_stride' in lib.tg_last_error_string()


def test_alignment_gates_of_the_backward_entries(lib, host):
    """tg_stack_time checked every source for 16-byte alignment and then cast y unchecked: TG_E_ARG now.
    tg_conv4x4s2_dgrad stores dx and reads act_y in 8-byte pairs in every form and checked neither: TG_E_ARG now.  The
    gates that existed are asserted next to them: the table of KERNELS.md, checked where no GPU is needed."""
    _, (a, b, c, d, e, f, g, h_) = host
    A = -2
    # tg_stack_time
    assert lib.tg_stack_time(arr(a, b, c), 3, d + 4, 2, 48, None) == A and b'alignment of y' in lib.tg_last_error_string()
    assert lib.tg_stack_time(arr(a, b, c), 3, d + 8, 2, 48, None) == A
    assert lib.tg_stack_time(arr(a, b + 4, c), 3, d, 2, 48, None) == A           # (one source of three: as before)
    assert lib.tg_stack_time(arr(a, b, c), 3, d, 2, 35, None) == A
    # tg_time_gather, tg_transpose01
    idx = (ctypes.c_int * 2)(1, 0)
    assert lib.tg_time_gather(a + 4, b, idx, 2, 3, 2, 48, None) == A and lib.tg_time_gather(a, b + 8, idx, 2, 3, 2, 48, None) == A
    assert lib.tg_time_gather(a, b, idx, 2, 3, 2, 35, None) == -1
    assert lib.tg_transpose01(a + 4, b, 3, 5, 48, None) == A and lib.tg_transpose01(a, b + 8, 3, 5, 48, None) == A
    assert lib.tg_transpose01(a, b, 3, 5, 35, None) == A
    # tg_depth_to_space_act_bwd: scale 2 | 4, w % 4 == 0, x, act_y, y 16-byte aligned
    for x_, ay, y_, w_, s_ in ((a + 4, b, c, 4, 2), (a, b + 8, c, 4, 2), (a, b, c + 4, 4, 2), (a, b, c, 5, 2), (a, b, c, 4, 3)):
        assert not lib.tg_depth_to_space_act_bwd_supported(x_, ay, y_, w_, s_)
        assert lib.tg_depth_to_space_act_bwd(x_, ay, 1, y_, 2, 3, 3, w_, s_, None) == A
    assert lib.tg_depth_to_space_act_bwd_supported(a, b, c, 4, 2) and lib.tg_depth_to_space_act_bwd(a, b, 0, c, 2, 3, 3, 4, 2, None) == A
    # tg_conv4x4s2_dgrad.  (2, 64, 64, 2, 64): one pass, 8-byte pairs; (2, 64, 128, 16, 16): split, 16-byte second pass
    assert lib.tg_conv4x4s2_workspace_floats(2, 64, 64, 2, 64, 1) == 0
    assert lib.tg_conv4x4s2_dgrad(a, b, None, 0, c + 4, None, 2, 64, 64, 2, 64, None) == A
    assert b'8-byte aligned' in lib.tg_last_error_string()
    assert lib.tg_conv4x4s2_dgrad(a, b, d + 4, 1, c, None, 2, 64, 64, 2, 64, None) == A
    assert lib.tg_conv4x4s2_dgrad(a, b, d + 12, 2, c + 8, None, 2, 64, 64, 2, 64, None) == A
    assert lib.tg_conv4x4s2_workspace_floats(2, 64, 128, 16, 16, 1) > 0
    assert lib.tg_conv4x4s2_dgrad(a, b, None, 0, c + 8, d, 2, 64, 128, 16, 16, None) == A
    assert b'16-byte aligned' in lib.tg_last_error_string()
    assert lib.tg_conv4x4s2_dgrad(a, b, None, 0, c, d + 8, 2, 64, 128, 16, 16, None) == A
    assert lib.tg_conv4x4s2_dgrad(a, b, e + 8, 1, c, d, 2, 64, 128, 16, 16, None) == A
    assert lib.tg_conv4x4s2_dgrad(a, b, None, 0, c, None, 2, 64, 128, 16, 16, None) == A      # the split form without a workspace


def test_conv4x4s2_dgrad_workspace_query_covers_the_restated_split(lib):
    """c4_dgrad_ksplit / c4_pick_ksplit restated: the partial sums are [ksplit][n][ci][h][w]."""
    def pick(base_wgs, nchunk):
        ks = 1
        while base_wgs * ks < 320 and ks * 2 <= nchunk // 2 and nchunk % (ks * 2) == 0:
            ks *= 2
        return ks
    split = set()
    for ci, co, h, w in G.CONV4_CASES:
        assert lib.tg_conv4x4s2_supported(N, ci, co, h, w)
        ks = 1 if w % 64 == 0 else pick((h // (8 if w == 32 else 16)) * (ci // 64) * N, co // 8)
        want = ks * N * ci * h * w if ks > 1 else 0
        assert lib.tg_conv4x4s2_workspace_floats(N, ci, co, h, w, 1) == want, (ci, co, h, w, ks)
        split.add((w % 64 == 0, ks > 1))
    assert split == {(True, False), (False, True)}          # the row-tile form; the small-map forms, split
