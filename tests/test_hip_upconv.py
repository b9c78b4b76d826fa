"""conv3x3(bilinear_x2(x)) with the matrix work at the low resolution (csrc/tg_upconv.hip) on the GPU.

  exact      integers in [-4, 4], weights +-1/2 (one tap at a time: every shift direction and border; then all taps), small
             integer bias: every product and sum is exact in fp32 (tests/test_upconv_cpu.py shows it for the torch
             statement), so the two launches must equal ops.upsample + ops.conv3x3 BIT FOR BIT, and the tap planes the
             torch statement's.  Maps 1x1 .. 17x40, one pixel past the GEMM's 128-pixel tile (3x43) and past the
             combine's 16 x 32 tile (17x33); n = 1 and 3; FNet's three channel pairs; no activation and LeakyReLU(0.2).
  random     uniform inputs at scales 1 and 1e2 against the fp64 CPU composition: max and mean error at most TWICE those
             of the composed GPU form on the same inputs (the bound tests/test_convt_z_wino.py uses for a re-ordered sum).
  placement  batch strides, unaligned bases and an output inside a larger buffer (tests/placement.py): guard words intact.
  plan       one child process with TG_UPCONV=1 (the switch is read once per process): flow-only plans and the frame
             plan against the oracle on poisoned workspaces, launch counts per kind equal to the default path's, the
             clip paths bit-equal among themselves.  The plan never replaces a reader that is a split-K pair (conv +
             finalize: that is what keeps the counts per kind equal), and at small maps most readers are
             (tg_conv3x3_pick_ksplit: 4-8 for all three at 16x24, 40x56 and 24x40).  So of the cases the issue names
             only 2 pairs of 70x120 run a factored reader (flow.0) in the plan; the 64x160 frame plan and the 70x120
             clip are added because flow.0 is a single launch there and runs factored in every part.  decoder2.0 and
             decoder3.0 run factored in a plan only at 134x320-class passes (bench.py's parity check and the output
             dumps of profiles/upconv.json cover those), and at every size through the ops above.
Every figure is printed before it is asserted.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import upconv_ref as R
from tests.placement import Arena, PLACEMENTS
from tests.test_upconv_cpu import PAIRS, exact_inputs

ROOT_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_DIR = os.path.join(ROOT_DIR, 'tests', 'golden')
MAPS = [(1, 1), (2, 3), (5, 7), (9, 33), (17, 40), (3, 43), (17, 33)]
MARK = 'UPCONV_PLAN_RECORD '


def _ops():
    from tecogan_pytorch_amd import ops, _lib
    return ops, _lib, _lib.lib()


def _composed_gpu(ops, x, wt, b, act):
    cout, cin = wt.shape[:2]
    pk, _, _, ocb = ops.pack_conv3x3(wt)
    return ops.conv3x3(ops.upsample(x, 2, ops.UP_BILINEAR), pk, b, cin, cout, ocb, act, ksplit=1)


@pytest.mark.parametrize('lrelu', [False, True], ids=['none', 'lrelu'])
@pytest.mark.parametrize('cin,cout', PAIRS)
def test_exact_arithmetic_is_bit_equal_to_the_composed_ops(cin, cout, lrelu):
    ops, _, _ = _ops()
    act = ops.ACT_LRELU02 if lrelu else ops.ACT_NONE
    bad = []
    for h, w in MAPS:
        for n in (1, 3):
            for weights in list(range(9)) + ['mixed']:
                x, wt, b = exact_inputs(cin, cout, h, w, n, weights)
                xd, wd, bd = x.cuda(), wt.cuda(), b.cuda()
                ap = ops.pack_upconv(wd)
                z = ops.upconv_tap_gemm(xd, ap, cin, cout)
                y = ops.upconv_combine(z, bd, cout, act)
                both = ops.upconv3x3(xd, ap, bd, cin, cout, act)
                want = _composed_gpu(ops, xd, wd, bd, act)
                ok = (torch.equal(z.cpu(), R.tap_planes(x, wt)), torch.equal(y, want), torch.equal(both, want),
                      torch.equal(y.cpu(), R.factored(x, wt, b, 0.2 if lrelu else None)))
                if not all(ok):
                    bad.append((h, w, n, weights, ok, (y - want).abs().max().item()))
    print('%d->%d %s: %d of %d cases differ' % (cin, cout, 'lrelu' if lrelu else 'none', len(bad), len(MAPS) * 2 * 10))
    assert not bad, bad[:5]


def test_the_pack_from_the_direct_forms_weights_is_the_pack_from_oihw():
    ops, _, _ = _ops()
    for cin, cout in PAIRS:
        wt = torch.randn(cout, cin, 3, 3, generator=torch.Generator().manual_seed(cin)).cuda()
        pk, _, _, ocb = ops.pack_conv3x3(wt)
        assert torch.equal(ops.pack_upconv(wt), ops.pack_upconv(pk, ocb=ocb, cin=cin, cout=cout)), (cin, cout)


@pytest.mark.parametrize('scale', [1.0, 1e2])
def test_random_inputs_stay_within_twice_the_composed_forms_error(scale):
    ops, _, _ = _ops()
    rows = []
    for cin, cout in PAIRS:
        for h, w in [(9, 33), (17, 40)]:
            g = torch.Generator().manual_seed(1000 + cin + h)
            x = (torch.rand(2, cin, h, w, generator=g) * 2 - 1) * scale
            wt = (torch.rand(cout, cin, 3, 3, generator=g) * 2 - 1) / (3 * cin ** 0.5)
            b = torch.rand(cout, generator=g) * 2 - 1
            ref = R.composed(x.double(), wt.double(), b.double(), 0.2)
            xd, wd, bd = x.cuda(), wt.cuda(), b.cuda()
            fac = ops.upconv3x3(xd, ops.pack_upconv(wd), bd, cin, cout, ops.ACT_LRELU02).cpu().double()
            com = _composed_gpu(ops, xd, wd, bd, ops.ACT_LRELU02).cpu().double()
            ef, ec = (fac - ref).abs(), (com - ref).abs()
            rows.append(dict(cin=cin, h=h, w=w, scale=scale, max_ratio=ef.max().item() / ec.max().item(),
                             mean_ratio=ef.mean().item() / ec.mean().item(), max_factored=ef.max().item(),
                             max_composed=ec.max().item()))
            print('scale %g %d->%d %dx%d: factored max %.3e mean %.3e, composed max %.3e mean %.3e, ratios %.2f %.2f' % (
                scale, cin, cout, h, w, ef.max(), ef.mean(), ec.max(), ec.mean(), rows[-1]['max_ratio'], rows[-1]['mean_ratio']))
    print('UPCONV_ERROR_RATIOS ' + json.dumps(rows))
    for r in rows:
        assert r['max_ratio'] <= 2.0 and r['mean_ratio'] <= 2.0, r


def test_two_launches_are_bit_identical():
    ops, _, _ = _ops()
    for cin, cout in PAIRS:
        x, wt, b = torch.rand(3, cin, 17, 40).cuda(), (torch.rand(cout, cin, 3, 3) - 0.5).cuda(), torch.rand(cout).cuda()
        ap = ops.pack_upconv(wt)
        first = ops.upconv3x3(x, ap, b, cin, cout, ops.ACT_LRELU02)
        for _ in range(2):
            assert torch.equal(ops.upconv3x3(x, ap, b, cin, cout, ops.ACT_LRELU02), first)


@pytest.mark.parametrize('name', sorted(PLACEMENTS))
@pytest.mark.parametrize('h,w', [(5, 7), (4, 8)], ids=['5x7', '4x8'])
def test_placement(name, h, w):
    """Every operand inside one guarded arena: offsets, batch strides with gaps, y a channel slice of a larger buffer."""
    ops, L, lib = _ops()
    off, extra, sliced = PLACEMENTS[name]
    cin, cout, n = 64, 32, 2
    x, wt, b = exact_inputs(cin, cout, h, w, n, 'mixed', seed=5)
    want = _composed_gpu(ops, x.cuda(), wt.cuda(), b.cuda(), ops.ACT_LRELU02).cpu()
    ap_src = ops.pack_upconv(wt.cuda()).cpu()
    a = Arena('cuda', margin_floats=1 << 15)
    xv = a.place(x, offset_floats=off, nstride=cin * h * w + extra, name='x')
    av = a.place(ap_src, name='a_packed')
    bv = a.place(b, offset_floats=off, name='bias')
    zv = a.out((n, 9 * cout, h, w), offset_floats=off, nstride=9 * cout * h * w + extra, name='z')
    yc = cout + 3 if sliced else cout
    yv = a.out((n, cout, 2 * h, 2 * w), offset_floats=off, nstride=yc * 4 * h * w + extra, name='y')
    st = torch.cuda.current_stream().cuda_stream
    L.check(lib.tg_upconv3x3_fwd(xv.data_ptr(), a.nstride(xv), av.data_ptr(), bv.data_ptr(), zv.data_ptr(), a.nstride(zv),
                                 yv.data_ptr(), a.nstride(yv), n, cin, cout, h, w, ops.ACT_LRELU02, st), 'tg_upconv3x3_fwd')
    torch.cuda.synchronize()
    a.check()
    a.finite(zv)
    a.finite(yv)
    assert torch.equal(zv.cpu(), R.tap_planes(x, wt))
    assert torch.equal(yv.cpu(), want)


def test_unsupported_arguments_are_refused_without_a_launch():
    ops, L, lib = _ops()
    cin, cout, n, h, w = 64, 32, 2, 4, 8
    a = Arena('cuda', margin_floats=1 << 15)
    xv = a.place(torch.rand(n, cin, h, w), name='x')
    av = a.place(torch.rand(9 * cin * cout), name='a_packed')
    odd = a.place(torch.rand(9 * cin * cout), offset_floats=1, name='a_packed + 4 bytes')
    bv = a.place(torch.rand(cout), name='bias')
    zv = a.out((n, 9 * cout, h, w), name='z')
    yv = a.out((n, cout, 2 * h, 2 * w), name='y')
    st = torch.cuda.current_stream().cuda_stream

    def call(x=xv, ap=av, z=zv, y=yv, n=n, cin=cin, cout=cout, h=h, w=w, act=ops.ACT_LRELU02, xns=None, zns=None, yns=None):
        return lib.tg_upconv3x3_fwd(x.data_ptr() if x is not None else None, a.nstride(xv) if xns is None else xns,
                                    ap.data_ptr() if ap is not None else None, bv.data_ptr(),
                                    z.data_ptr() if z is not None else None, a.nstride(zv) if zns is None else zns,
                                    y.data_ptr() if y is not None else None, a.nstride(yv) if yns is None else yns,
                                    n, cin, cout, h, w, act, st)
    for kw in (dict(cin=64, cout=64), dict(cin=32, cout=16), dict(cin=96, cout=48), dict(cin=128, cout=32), dict(cin=512, cout=256),
               dict(n=0), dict(h=0), dict(w=-1), dict(x=None), dict(ap=None), dict(z=None), dict(y=None), dict(ap=odd),
               dict(h=1 << 12, w=1 << 12)):
        assert call(**kw) == L.TG_E_ARG, kw
    assert lib.tg_upconv_combine(zv.data_ptr(), a.nstride(zv), bv.data_ptr(), yv.data_ptr(), a.nstride(yv), n, cout, h, w, 9,
                                 st) == L.TG_E_ARG
    for kw in (dict(xns=cin * h * w - 1), dict(zns=9 * cout * h * w - 1), dict(yns=cout * 4 * h * w - 1)):
        assert call(**kw) == L.TG_E_SHAPE, kw       # the batch-stride contract of every entry
    torch.cuda.synchronize()
    a.check(outputs_untouched=True)


# ---- the frame plan, in one child process with TG_UPCONV=1 ------------------------------------------------------------
FLOW_ONLY = [(2, 16, 24), (3, 40, 56), (2, 70, 120)]      # (pairs, h, w): source maps down to 2x3; 5x7, 10x14, 20x28; 8x15 ..
FRAME = (24, 40)
# Beside the cases above, the smallest shapes at which a reader of the plan IS a single launch and therefore runs factored
# in every part below (flow.0: one pair from 64x160 on, two or three pairs at 70x120)
FRAME_FACTORED = (64, 160)
CLIPS = [FRAME, (70, 120)]


def _cases():
    from tests import plan_matrix as M
    flow = [M._c('upconv_fnet%d_%dx%d' % (k, h, w), 64, 1, 4, 'BD', 1, h, w, {}, fnet_only=k, frame_body='layers')
            for k, h, w in FLOW_ONLY]
    return flow, [M._c('upconv_frame_%dx%d' % f, 64, 1, 4, 'BD', 1, f[0], f[1], {}) for f in (FRAME, FRAME_FACTORED)]


def child_main():
    """TG_UPCONV=1 and TG_FNET_BATCH=2 are in this process's environment.  One JSON line per part; ends at the first
    part that raises."""
    from procedural_weights import smooth_clip
    from tests import test_hip_plan_matrix as PM
    ops, L, lib = _ops()
    flow, frames = _cases()
    for c in flow:
        k, h, w = c.extra['fnet_only'], c.h, c.w
        rec = PM.run_flow_only(c)
        rec.update(name=c.name, prefers=[lib.tg_upconv_prefers(k, ci, co, (h // 8) << i, (w // 8) << i)
                                         for i, (ci, co) in enumerate(reversed(PAIRS))])
        print(MARK + json.dumps(rec), flush=True)
    for frame in frames:
        rec = PM.run_frames(frame)
        rec.update(name=frame.name)
        print(MARK + json.dumps(rec), flush=True)
    net = PM.make_net(frames[0])
    for h, w in CLIPS:
        clip = smooth_clip(9, 3, h, w, seed=31)
        first = net.infer_sequence(clip, 'cuda', pipeline=True)
        again = net.infer_sequence(clip, 'cuda', pipeline=True)
        one = net.infer_sequence(clip, 'cuda', pipeline='one_stream')
        streamed = np.concatenate([chunk.copy() for chunk in net.infer_stream((f for f in clip), 'cuda')], 0)
        d = np.abs(net.infer_sequence(clip, 'cuda', pipeline=False).astype(np.int16) - first.astype(np.int16))
        print(MARK + json.dumps(dict(name='clip_%dx%d' % (h, w), repeat=bool(np.array_equal(first, again)),
                                     one_stream=bool(np.array_equal(first, one)), stream=bool(np.array_equal(first, streamed)),
                                     max_level=int(d.max()), differing=float((d > 0).mean()))), flush=True)


@pytest.fixture(scope='module')
def plan_records():
    env = {k: v for k, v in os.environ.items() if k not in ('TG_CONV_WINO', 'TG_WINO_CHAIN', 'TG_WINO_RES', 'TG_WINO_RES_CT')}
    env.update(TG_UPCONV='1', TG_FNET_BATCH='2')
    script = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
              "from tests.test_hip_upconv import child_main\nchild_main()\n" % (ROOT_DIR, GOLDEN_DIR))
    r = subprocess.run([sys.executable, '-c', script], env=env, capture_output=True, text=True, timeout=600)
    recs = {}
    for line in r.stdout.splitlines():
        if line.startswith(MARK):
            d = json.loads(line[len(MARK):])
            recs[d['name']] = d
            print(line[:600])
    assert r.returncode == 0, 'the TG_UPCONV=1 child ended with status %d\n%s\n%s' % (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return recs


def _default_stats(c):
    """Launches per kind of the same plan under the default rule (this process; the rule never picks these small maps)."""
    from tests import test_hip_plan_matrix as PM
    k = c.extra.get('fnet_only')
    p = PM.Poisoned(PM.make_net(c), k or c.n, c.h, c.w, fnet_only=bool(k))
    return p.stats()


@pytest.mark.parametrize('i', range(len(FLOW_ONLY) + 2), ids=['%dx%dx%d' % c for c in FLOW_ONLY] + ['frame_%dx%d' % f for f in (FRAME, FRAME_FACTORED)])
def test_plan_with_the_factored_readers(i, plan_records):
    from tests import plan_matrix as M
    _, _, lib = _ops()
    flow, frames = _cases()
    c = (flow + frames)[i]
    rec = plan_records[c.name]
    print(c.name, 'flow err', rec['flow_err'], 'frame err', rec['frame_err'], 'prefers', rec.get('prefers'))
    if 'prefers' in rec:
        assert rec['prefers'] == [1, 1, 1]
        k = c.extra['fnet_only']
        assert [lib.tg_upconv_prefers(k, ci, co, (c.h // 8) << j, (c.w // 8) << j) for j, (ci, co) in enumerate(reversed(PAIRS))] \
            == [0, 0, 0], 'the default rule picks the factored form at a test-sized map'
    assert max(rec['flow_err']) <= M.FLOW_TOL and max(rec['frame_err']) <= M.FRAME_TOL, (rec['flow_err'], rec['frame_err'])
    assert rec['finite'] and rec['payload_words'] == 0, 'scratch read before it was written, or output not written'
    assert rec['band_ok'], 'a launch wrote behind tg_frnet_workspace_floats'
    assert rec['repeat_equal'], 'the second step on the used workspace differs from the first'
    assert rec['stats'] == _default_stats(c), (rec['stats'], _default_stats(c))


@pytest.mark.parametrize('h,w', CLIPS)
def test_clip_paths_agree_with_the_factored_readers(h, w, plan_records):
    rec = plan_records['clip_%dx%d' % (h, w)]
    print('TG_UPCONV=1, TG_FNET_BATCH=2, 9 frames of %dx%d: %s' % (h, w, rec))
    assert rec['repeat'] and rec['one_stream'] and rec['stream'], rec
    assert rec['max_level'] <= 1 and rec['differing'] <= 2e-3, rec
