"""The frame-plan matrix without a GPU (tests/plan_matrix.py is the table, tests/test_hip_plan_matrix.py runs it):

  * the table covers every launch kind the plan knows, and every default-rule case sits on the side of each threshold
    its claims name -- asked of the library's own host functions where it exports the rule, restated from the code
    where it does not;
  * the bound the GPU test uses has teeth: three defects of the kind a launch-list bug makes, planted in the oracle,
    each move the frame by at least ten times that bound, for every configuration of the table;
  * the plan refuses out_nc != in_nc, and sizes the tap-plane region of the fused HR stage for nf < 32.

Measured separation (max |defective - clean| over the frame, smallest and largest over the 16 configurations, inputs as
in the GPU test: a smooth clip, frame 1 warping a textured hr_prev): see DESIGN.md section 7m.
"""
import ctypes

import pytest
import torch

import tecogan_pytorch_amd  # noqa: F401
from tecogan_pytorch_amd import _lib as L
from oracle import tecogan_oracle as O
from procedural_weights import generator_state_dict, smooth_clip

from tests import plan_matrix as M


def _kind_names():
    lib = L.lib()
    return [lib.tg_frnet_kind_name(k).decode() for k in range(lib.tg_frnet_plan_kinds())]


def test_table_covers_every_launch_kind():
    names = _kind_names()
    reached = set()
    for c in M.CASES:
        assert set(c.expect) <= set(names), (c.name, set(c.expect) - set(names))
        reached |= {k for k, v in c.expect.items() if v > 0}
    assert not reached & set(M.NOT_REACHED), reached & set(M.NOT_REACHED)
    missing = set(names) - reached - set(M.NOT_REACHED)
    assert not missing, f'no case reaches {sorted(missing)}'
    assert reached | set(M.NOT_REACHED) == set(names)


def test_table_rules():
    """Sizes, configurations and shapes the table must hold."""
    for c in M.CASES:
        assert c.h * c.w <= M.MAX_FRAME_PIXELS, c.name
        assert c.h >= 8 and c.w >= 8 and c.nb >= 1 and c.precision in ('fp32', 'fp16'), c.name
        assert set(c.env) <= {'TG_CONV_WINO', 'TG_WINO_CHAIN', 'TG_WINO_RES', 'TG_WINO_RES_CT'}, c.name
        assert c.extra['body'] in ('resident', 'chain', 'layers'), c.name
        assert (c.extra['body'] == 'resident') == (c.expect.get(M.RES, 0) == 1), c.name
        assert (c.extra['body'] == 'chain') == (c.expect.get(M.CHAIN, 0) == 1), c.name
        assert ('frame_body' in c.extra) == bool(c.extra.get('fnet_only')), c.name
        assert c.extra.get('frame_body', 'layers') in ('resident', 'chain', 'layers') and (c.n == 1 or 'frame_body' not in c.extra), c.name
    fp32 = [c for c in M.CASES if c.precision == 'fp32']
    assert {c.nf for c in fp32} == {64, 48, 32}
    assert {c.nb for c in fp32} >= {1, 2, 10, 11, 12}
    assert {(c.scale, c.degradation) for c in fp32} == {(4, 'BD'), (2, 'BI'), (2, 'BD'), (4, 'BI')}
    assert sorted(c.scale for c in M.CASES if c.precision == 'fp16') == [2, 4]
    assert {c.extra.get('fnet_only') for c in M.CASES} >= {2, 8}
    default = [c for c in fp32 if not c.env]
    # an odd map at each FNet level (h or w odd after 0, 1 and 2 poolings), and flows that need the reflect pad
    for lvl in range(3):
        assert any(((c.h >> lvl) % 2 or (c.w >> lvl) % 2) for c in default), lvl
    assert any(c.h % 8 for c in default) and any(c.w % 8 for c in default)
    # uint8 frames for n > 1 and for the one-pixel tail (HR width no multiple of 4)
    assert any(c.extra.get('u8') and c.n > 1 for c in default)
    assert any(c.extra.get('u8') and (c.scale * c.w) % 4 for c in default)
    for s in (2, 4):
        assert sum(1 for c in M.CASES if c.extra.get('phases') and c.scale == s and c.n == 1) >= 1


# ---- the claims: (rule, args..., answer) ------------------------------------------------------------------------------
def _zsplit(strips_rows, tiles_x, band):
    """Two launches: whole rounds of the 512 resident slots (2 a CU, 256 CUs) and a remainder."""
    slots = 512
    wgs = tiles_x * strips_rows
    if wgs < slots:
        return False
    rows1 = (wgs // slots) * slots // tiles_x
    if not 1 <= rows1 < strips_rows:
        return False
    rem = wgs % slots
    return band is None or (4 * rem >= slots and 100 * rem <= 95 * slots)


def _claim(lib, c, claim):
    rule, args, ans = claim[0], claim[1:-1], claim[-1]
    zh, zw = c.scale * c.h // 2, c.scale * c.w // 2
    if rule == 'wino':
        return lib.tg_conv3x3_prefers_wino(*args) == ans
    if rule == 'wgs':
        h, w = args
        return c.n * M.cdiv(h, 2) * M.cdiv(w, 32) == ans and (h, w) == (c.h, c.w)
    if rule == 'tiles':
        return (768 < M.body_tiles(c) <= 3000) == bool(ans)
    if rule == 'tiles_n':
        return (768 < M.body_tiles(c._replace(n=args[0])) <= 3000) == bool(ans)
    if rule == 'layers':
        return M.body_layers(c) == ans
    if rule == 'layers_fit':
        return (2 <= M.body_layers(c) <= 24) == bool(ans)
    if rule == 'resident_shape':
        shape = c.n == 1 and c.nf == 64 and c.h % 2 == 0 and c.w % 2 == 0
        # (a refusal for the shape needs no device; an admission also asks for the CU count)
        return shape == bool(ans) and (shape or lib.tg_conv3x3_wino_resident_supported(c.n, c.nf, c.h, c.w) == 0)
    if rule == 'rows4':
        return (c.n * c.h * c.w >= 200000) == bool(ans)
    if rule == 'ksplit':
        return lib.tg_conv3x3_pick_ksplit(*args) == ans
    if rule == 'ksplit_gt1':
        return lib.tg_conv3x3_pick_ksplit(*args) > 1
    if rule == 'wg_ksplit':
        cin, cout, h, w = args
        return (c.n * M.cdiv(w, 32) * M.cdiv(h, 2) * M.cdiv(cout, 64) <= 128 and M.cdiv(cin, 8) >= 6 and
                c.n * h * w < 200000) == bool(ans)
    if rule == 'zsplit_wino':
        return (c.nf == 64 and c.n == 1 and _zsplit(M.cdiv(zh, 2), M.cdiv(zw, 32), None)) == bool(ans)
    if rule == 'zsplit_direct':
        return (c.nf < 64 and c.n == 1 and _zsplit(M.cdiv(zh, 4), M.cdiv(zw, 32), 'band')) == bool(ans)
    if rule == 'w4':
        return ((c.scale * c.w) % 4 == 0) == bool(ans)
    raise AssertionError(f'unknown rule {rule}')


def test_default_rule_cases_sit_where_their_claims_say():
    """(The library reads its switches once per process: with one of them set in the caller's environment the claims,
    which are about the default rule, are checked in a child process without it.)"""
    import os
    import subprocess
    import sys
    switches = ('TG_CONV_WINO', 'TG_WINO_CHAIN', 'TG_WINO_RES')
    if any(k in os.environ for k in switches):
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        script = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
                  "from tests.test_plan_matrix_cpu import check_claims; check_claims()\n"
                  % (root, os.path.join(root, 'tests', 'golden')))
        env = {k: v for k, v in os.environ.items() if k not in switches}
        subprocess.run([sys.executable, '-c', script], check=True, env=env, timeout=300)
    else:
        check_claims()


def check_claims():
    lib = L.lib()
    nclaims = 0
    for c in M.CASES:
        if c.env:
            assert not c.extra['claims'], c.name
            continue
        for claim in c.extra['claims']:
            assert _claim(lib, c, claim), (c.name, claim)
            nclaims += 1
        # what every default-rule case's body says about itself
        body_wino = lib.tg_conv3x3_prefers_wino(c.n, c.nf, c.nf, c.h, c.w) == 1
        # (a flow-only case's n, h, w are those of the frame plan that consumes its flows: frame_body is about that plan)
        if c.precision == 'fp32':
            fits = 2 <= M.body_layers(c) <= 24
            resident = body_wino and fits and c.n == 1 and c.nf == 64 and c.h % 2 == 0 and c.w % 2 == 0
            chain = body_wino and fits and 768 < M.body_tiles(c) <= 3000
            want = 'resident' if resident else ('chain' if chain else 'layers')
            assert c.extra['frame_body' if c.extra.get('fnet_only') else 'body'] == want, (c.name, want)
    assert nclaims >= 60


# ---- the refusals --------------------------------------------------------------------------------------------------------
def _cfg(**kw):
    d = dict(in_nc=3, out_nc=3, nf=64, nb=10, scale=4, up_mode=1, n=1, h=64, w=160, fnet_only=0)
    d.update(kw)
    return L.FrnetCfg(d['in_nc'], d['out_nc'], d['nf'], d['nb'], d['scale'], d['up_mode'], d['n'], d['h'], d['w'], d['fnet_only'])


@pytest.mark.parametrize('out_nc', [1, 2, 4])
def test_plan_refuses_out_nc_other_than_in_nc(out_nc):
    """The frame is the next call's hr_prev (read as in_nc channels) and the output conv adds the up-sampled lr_curr
    channel by channel (out_nc of them per image): out_nc = 4 would read past lr_curr, out_nc < 3 the wrong image."""
    from tests.test_abi_cpu import test_frame_plan_refuses_out_nc_other_than_in_nc as refusal
    lib = L.lib()
    assert lib.tg_frnet_workspace_floats(ctypes.byref(_cfg())) > 0           # the same shape with out_nc = 3 is admitted
    for scale, n in ((4, 1), (2, 3)):
        bad = _cfg(out_nc=out_nc, scale=scale, n=n)
        assert lib.tg_frnet_workspace_floats(ctypes.byref(bad)) == 0
        assert lib.tg_frnet_f16_workspace_bytes(ctypes.byref(bad)) == 0
    refusal(out_nc)                                                          # the size queries and plan creation at 134x320


def test_workspace_holds_the_tap_planes_for_nf_below_32():
    """The fused HR stage writes 9 * out_nc = 27 tap planes per image at a batch stride of 32 planes into the region
    of the last nf-channel HR tensor (U2 at 4x, U1 at 2x): the region is sized for max(nf, 32) planes.  At 64x160 no
    SRNet layer splits K, so nothing else of the carve depends on nf."""
    lib = L.lib()
    ws = lambda **kw: lib.tg_frnet_workspace_floats(ctypes.byref(_cfg(nb=2, **kw)))      # noqa: E731
    for n in (1, 3):
        hw = 64 * 160
        assert ws(nf=16, scale=2, n=n) == ws(nf=32, scale=2, n=n)                     # U1 is the plane region
        assert ws(nf=16, scale=4, n=n) == ws(nf=32, scale=4, n=n) - n * 16 * 4 * hw   # U2 is; U1 holds 4 nf planes
        assert ws(nf=48, scale=4, n=n) == ws(nf=32, scale=4, n=n) + n * 16 * 20 * hw


# ---- the bound has teeth -------------------------------------------------------------------------------------------------
def _frame_inputs(n, s, h, w):
    """Frame 1 of the GPU test: lr_curr, lr_prev of a smooth clip and a textured hr_prev."""
    clips = [smooth_clip(2, 3, h, w, seed=11 + i) for i in range(n)]
    lc = torch.stack([c[1] for c in clips])
    lp = torch.stack([c[0] for c in clips])
    hp = torch.stack([smooth_clip(1, 3, s * h, s * w, seed=31 + i, shift=0.0)[0] for i in range(n)])
    return lc, lp, hp


class _Defects:
    """The three defects, planted through the two functions the oracle's forward passes call."""

    def __init__(self, which, nb):
        self.which, self.block, self.pool_calls, self.kept = which, nb // 2, 0, None

    def conv(self, orig):
        def f(x, sd, key, pad=1, stride=1):
            y = orig(x, sd, key, pad, stride)
            if self.which == 'halo' and key == f'resblocks.{self.block}.conv.0':
                # the last output row as if the row above it (another tile's, the halo) had been zero
                x0 = x.clone()
                x0[:, :, -2] = 0
                y = y.clone()
                y[:, :, -1] = orig(x0, sd, key, pad, stride)[:, :, -1]
            if self.which == 'residual':
                if key == f'resblocks.{self.block}.conv.0':
                    self.kept = x
                elif key == f'resblocks.{self.block}.conv.2':
                    y = y - self.kept         # the caller adds it back: the block's output is conv2 alone
            return y
        return f

    def pool(self, orig):
        def f(x, *a, **kw):
            y = orig(x, *a, **kw)
            self.pool_calls += 1
            if self.which == 'pool' and self.pool_calls == 1:
                y = y.clone()
                y[:, :, -1] = 0               # the pooled map's last row never written (zero pages)
            return y
        return f


@pytest.mark.parametrize('cfg', sorted(M.configs().items()), ids=lambda kv: 'nf%d_nb%d_%dx%s_%dx%d' % (kv[0] + kv[1]))
def test_each_defect_moves_the_frame_by_ten_times_the_bound(cfg, monkeypatch):
    (nf, nb, s, deg), (h, w) = cfg
    torch.set_num_threads(min(16, torch.get_num_threads()))
    sd = generator_state_dict(nf=nf, nb=nb, scale=s, degradation=deg)
    lc, lp, hp = _frame_inputs(1, s, h, w)
    with torch.no_grad():
        clean = O.frnet_step(sd, lc, lp, hp, s, deg)
        moved = {}
        for which in ('halo', 'residual', 'pool'):
            d = _Defects(which, nb)
            with monkeypatch.context() as m:
                m.setattr(O, '_conv', d.conv(O._conv))
                m.setattr(O.F, 'max_pool2d', d.pool(O.F.max_pool2d))
                bad = O.frnet_step(sd, lc, lp, hp, s, deg)
            assert which != 'pool' or d.pool_calls == 3
            moved[which] = (bad - clean).abs().max().item()
    print('defect separation nf=%d nb=%d %dx%s %dx%d: ' % (nf, nb, s, deg, h, w) +
          ' '.join('%s=%.3e' % kv for kv in moved.items()))
    for which, e in moved.items():
        assert e >= 10 * M.FRAME_TOL, (which, e)
