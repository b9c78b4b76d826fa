"""The frame plan (tg_frnet_step and its siblings) at every launch-list decision of tests/plan_matrix.py, each case on a
POISONED workspace and against the CPU oracle.

Per case, on a fresh plan:

  branch     tg_frnet_plan_kind_stats equals the case's `expect`; chain_state() after the run is (0, True) where a
             one-launch body is expected and (0, False) where it is not.
  poison     tg_frnet_workspace_floats / tg_frnet_f16_workspace_bytes are wrapped while the plan is created, so that its
             allocation carries a guard band behind what the library asked for; the whole allocation is filled with
             placement.pattern(1) words (0xFF bytes for the fp16 workspace) before the first step.  The output must be
             finite (a guard word is a NaN with a payload: scratch read before it is written shows), the band bit for
             bit as it was (the size query is enough), and a second step on the now-used workspace equal bit for bit.
  reference  two recurrent frames of a smooth clip against oracle.frnet_step: frame 0 from the zero state, frame 1 from the
             GPU's own frame 0 on both sides; the flow read back through tg_frnet_plan_flow against the oracle's.  Bounds:
             the project's own (top of tests/test_hip_parity.py), 1e-4 for the frame, 2e-4 for the flow -- not fitted to
             this run; tests/test_plan_matrix_cpu.py shows what they catch.
  uint8      the bytes equal oracle.float32_to_uint8 of the fp32 frame the same call wrote.
  digest     SHA-256 over the bytes of both fp32 frames, both flows (a flow-only case: its flows and frames) and the uint8
             frames where the case asks for them: recorded, not asserted -- two libraries compute the same when a run
             of each gives the same digests (profiles/frame_plan_refactor.json is such a comparison).
  phases     (flagged cases) tg_frnet_step_phase(1, slot) + (2, slot), both slots, and tg_frnet_step_srnet fed from a
             flow-only plan of one pair, equal tg_frnet_step bit for bit; the flow-only cases feed tg_frnet_step_srnet
             from a batched flow pass, every frame within the bounds above.

The forcing switches are read once per process: the cases are grouped by `env`, every group with switches runs in ONE
child process (one at a time, with a timeout) that prints a JSON line per case; the default-rule group runs in-process.
Every figure is printed before anything is asserted; TG_PLAN_MATRIX_JSON=<path> also collects the records in a file
(profiles/plan_matrix.json is such a run).
"""
import contextlib
import ctypes
import hashlib
import json
import os
import subprocess
import sys
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import tecogan_oracle as O
from procedural_weights import generator_state_dict, smooth_clip

from tests import plan_matrix as M
from tests.placement import GUARD, pattern

ROOT_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_DIR = os.path.join(ROOT_DIR, 'tests', 'golden')
SWITCHES = ('TG_CONV_WINO', 'TG_WINO_CHAIN', 'TG_WINO_RES', 'TG_WINO_RES_CT')
BAND_WORDS = 1 << 16            # guard band behind the fp32 workspace (and as many bytes behind the fp16 one)
MARK = 'PLAN_MATRIX_RECORD '
DEV = 'cuda:0'


# ---- plumbing -------------------------------------------------------------------------------------------------------------
def _lib():
    from tecogan_pytorch_amd import _lib
    return _lib, _lib.lib()


@contextlib.contextmanager
def guard_band(asked):
    """While active, both size queries answer BAND_WORDS more than the library needs; `asked` collects what it needs."""
    _, lib = _lib()
    f32, f16 = lib.tg_frnet_workspace_floats, lib.tg_frnet_f16_workspace_bytes

    def floats(cfg):
        v = f32(cfg)
        asked.append(('f32', v))
        return v + BAND_WORDS if v else 0

    def halves(cfg):
        v = f16(cfg)
        asked.append(('f16', v))
        return v + BAND_WORDS if v else 0
    lib.tg_frnet_workspace_floats, lib.tg_frnet_f16_workspace_bytes = floats, halves
    try:
        yield
    finally:
        lib.tg_frnet_workspace_floats, lib.tg_frnet_f16_workspace_bytes = f32, f16


_SD = {}


def weights(c):
    k = (c.nf, c.nb, c.scale, c.degradation)
    if k not in _SD:
        _SD[k] = generator_state_dict(nf=c.nf, nb=c.nb, scale=c.scale, degradation=c.degradation)
    return _SD[k]


def make_net(c):
    from tecogan_pytorch_amd.models.networks import FRNet
    net = FRNet(3, 3, c.nf, c.nb, c.degradation, c.scale, precision=c.precision)
    net.load_state_dict(weights(c), strict=True)
    return net.to(DEV).eval()


class Poisoned:
    """A fresh plan whose workspaces carry a guard band and are poisoned before the first step."""

    def __init__(self, net, n, h, w, fnet_only=False):
        asked = []
        with guard_band(asked):
            self.plan = net._get_plan(n, h, w, torch.device(DEV), fnet_only=fnet_only)
        self.handle = self.plan.handle
        self.need = dict(asked)
        ws = self.plan.workspace
        assert ws.numel() == self.need['f32'] + BAND_WORDS and self.need['f32'] > 0
        self.words = ws.view(torch.int32)
        self.words.fill_(pattern(1))
        self.h16 = getattr(self.plan, 'workspace_f16', None)
        if self.h16 is not None:
            assert self.h16.numel() == self.need['f16'] + BAND_WORDS
            self.h16.fill_(0xFF)

    def band_ok(self):
        ok = bool((self.words[self.need['f32']:] == pattern(1)).all().item())
        if self.h16 is not None:
            ok = ok and bool((self.h16[self.need['f16']:] == 0xFF).all().item())
        return ok

    def flow(self, slot, n, fh, fw):
        _, lib = _lib()
        ptr = lib.tg_frnet_plan_flow(self.handle, slot)
        off = (ptr - self.plan.workspace.data_ptr()) // 4
        assert 0 <= off and off + n * 2 * fh * fw <= self.need['f32']
        return self.plan.workspace[off:off + n * 2 * fh * fw].view(n, 2, fh, fw).clone()

    def stats(self):
        L, lib = _lib()
        out = {}
        for k in range(lib.tg_frnet_plan_kinds()):
            v = ctypes.c_int()
            L.check(lib.tg_frnet_plan_kind_stats(self.handle, k, ctypes.byref(v), None, None), 'kind_stats')
            out[lib.tg_frnet_kind_name(k).decode()] = v.value
        return out


def fresh_out(n, c, h, w):
    """An output that starts as guard words of slot 2: an element never written is a NaN with that payload."""
    t = torch.empty(n, c, h, w, dtype=torch.float32, device=DEV)
    t.view(torch.int32).fill_(pattern(2))
    return t


def payload_words(t):
    """Elements of `t` that are guard words of any slot."""
    return int(((t.view(torch.int32) & ~0xFF) == GUARD).sum().item())


def stream():
    return torch.cuda.current_stream().cuda_stream


def step(p, lc, lp, hp, out, u8=None):
    L, lib = _lib()
    L.check(lib.tg_frnet_step(p.handle, lc.data_ptr(), lp.data_ptr(), hp.data_ptr(), out.data_ptr(),
                              None if u8 is None else u8.data_ptr(), stream()), 'tg_frnet_step')


def u8_mismatches(u8, out):
    want = O.float32_to_uint8(out.cpu().permute(0, 2, 3, 1).contiguous().numpy())
    return int((u8.cpu().numpy() != want).sum())


def err(a, b):
    return (a.detach().cpu().double() - b.detach().cpu().double()).abs().max().item()


def digest(*tensors):
    """SHA-256 over the bytes of the tensors, in this order (None: not asked for)."""
    h = hashlib.sha256()
    for t in tensors:
        if t is not None:
            h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def clips(c, frames):
    return [smooth_clip(frames, 3, c.h, c.w, seed=11 + i) for i in range(c.n)]


# ---- one case ---------------------------------------------------------------------------------------------------------------
def run_case(c):
    """Runs the case and returns its record: figures and outcomes, nothing asserted (check_record does that)."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    t0 = time.time()
    rec = run_flow_only(c) if c.extra.get('fnet_only') else run_frames(c)
    torch.cuda.synchronize()
    rec.update(name=c.name, wall_s=round(time.time() - t0, 2))
    return rec


def run_frames(c):
    s, n, h, w = c.scale, c.n, c.h, c.w
    fh, fw = h // 8 * 8, w // 8 * 8
    sd, net = weights(c), make_net(c)
    p = Poisoned(net, n, h, w)
    rec = dict(stats=p.stats(), workspace_floats=p.need['f32'])
    cl = clips(c, 2)
    lr0 = torch.stack([x[0] for x in cl]).to(DEV)
    lr1 = torch.stack([x[1] for x in cl]).to(DEV)
    zl, zh = torch.zeros_like(lr0), torch.zeros(n, 3, s * h, s * w, device=DEV)
    want_u8 = bool(c.extra.get('u8'))
    mk8 = (lambda: torch.full((n, s * h, s * w, 3), 0x5A, dtype=torch.uint8, device=DEV)) if want_u8 else (lambda: None)

    out0, b0 = fresh_out(n, 3, s * h, s * w), mk8()
    step(p, lr0, zl, zh, out0, b0)
    torch.cuda.synchronize()
    flow0 = p.flow(0, n, fh, fw)
    rec['band_ok'] = p.band_ok()
    again, b0b = fresh_out(n, 3, s * h, s * w), mk8()
    step(p, lr0, zl, zh, again, b0b)                       # the same frame on the now-used workspace
    out1, b1 = fresh_out(n, 3, s * h, s * w), mk8()
    step(p, lr1, lr0, out0, out1, b1)
    torch.cuda.synchronize()
    flow1 = p.flow(0, n, fh, fw)
    p.plan.check_chain()
    rec['chain_state'] = list(p.plan.chain_state())
    rec['band_ok'] = rec['band_ok'] and p.band_ok()
    rec['finite'] = bool(torch.isfinite(out0).all().item() and torch.isfinite(out1).all().item() and
                         torch.isfinite(flow0).all().item() and torch.isfinite(flow1).all().item())
    rec['payload_words'] = payload_words(out0) + payload_words(out1) + payload_words(flow0) + payload_words(flow1)
    rec['repeat_equal'] = bool(torch.equal(out0.view(torch.int32), again.view(torch.int32)) and
                               (not want_u8 or torch.equal(b0, b0b)))
    rec['digest'] = digest(out0, out1, flow0, flow1, b0, b1)
    if want_u8:
        rec['u8_mismatches'] = u8_mismatches(b0, out0) + u8_mismatches(b1, out1)
    if c.precision == 'fp32':
        with torch.no_grad():
            ref0, parts0 = O.frnet_step(sd, lr0.cpu(), zl.cpu(), zh.cpu(), s, c.degradation, return_parts=True)
            ref1, parts1 = O.frnet_step(sd, lr1.cpu(), lr0.cpu(), out0.cpu(), s, c.degradation, return_parts=True)
        rec['frame_err'] = [err(out0, ref0), err(out1, ref1)]
        rec['flow_err'] = [err(flow0, parts0['lr_flow']), err(flow1, parts1['lr_flow'])]
    if c.extra.get('phases'):
        L, lib = _lib()
        eq = {}
        for slot in (0, 1):
            o = fresh_out(n, 3, s * h, s * w)
            L.check(lib.tg_frnet_step_phase(p.handle, 1, slot, lr1.data_ptr(), lr0.data_ptr(), None, None, None, stream()), 'phase 1')
            L.check(lib.tg_frnet_step_phase(p.handle, 2, slot, lr1.data_ptr(), None, out0.data_ptr(), o.data_ptr(), None, stream()), 'phase 2')
            torch.cuda.synchronize()
            eq['slot%d' % slot] = bool(torch.equal(o.view(torch.int32), out1.view(torch.int32)))
        fp = Poisoned(net, 1, h, w, fnet_only=True)
        L.check(lib.tg_frnet_step_phase(fp.handle, 1, 0, lr1.data_ptr(), lr0.data_ptr(), None, None, None, stream()), 'flow pass')
        o = fresh_out(n, 3, s * h, s * w)
        L.check(lib.tg_frnet_step_srnet(p.handle, lib.tg_frnet_plan_flow(fp.handle, 0), lr1.data_ptr(), out0.data_ptr(),
                                        o.data_ptr(), None, stream()), 'tg_frnet_step_srnet')
        torch.cuda.synchronize()
        eq['srnet'] = bool(torch.equal(o.view(torch.int32), out1.view(torch.int32)))
        eq['flow_plan_band_ok'] = fp.band_ok()
        p.plan.check_chain()
        rec['phases_equal'] = eq
        rec['band_ok'] = rec['band_ok'] and p.band_ok()
    return rec


def run_flow_only(c):
    """A flow-only plan of k frame pairs feeds tg_frnet_step_srnet on the frame plan of one frame."""
    L, lib = _lib()
    s, h, w, k = c.scale, c.h, c.w, c.extra['fnet_only']
    fh, fw = h // 8 * 8, w // 8 * 8
    sd, net = weights(c), make_net(c)
    fp = Poisoned(net, k, h, w, fnet_only=True)
    p = Poisoned(net, 1, h, w)
    rec = dict(stats=fp.stats(), workspace_floats=fp.need['f32'])
    clip = smooth_clip(k + 1, 3, h, w, seed=17).to(DEV)
    hp = smooth_clip(1, 3, s * h, s * w, seed=31, shift=0.0).to(DEV)
    L.check(lib.tg_frnet_step_phase(fp.handle, 1, 1, clip[1:].data_ptr(), clip[:k].data_ptr(), None, None, None, stream()), 'flow pass')
    torch.cuda.synchronize()
    flows = fp.flow(1, k, fh, fw)
    L.check(lib.tg_frnet_step_phase(fp.handle, 1, 1, clip[1:].data_ptr(), clip[:k].data_ptr(), None, None, None, stream()), 'flow pass')
    torch.cuda.synchronize()
    again = fp.flow(1, k, fh, fw)
    base = lib.tg_frnet_plan_flow(fp.handle, 1)
    outs = []
    for j in range(k):
        o = fresh_out(1, 3, s * h, s * w)
        L.check(lib.tg_frnet_step_srnet(p.handle, base + j * 2 * fh * fw * 4, clip[j + 1:j + 2].data_ptr(), hp.data_ptr(),
                                        o.data_ptr(), None, stream()), 'tg_frnet_step_srnet')
        outs.append(o)
    torch.cuda.synchronize()
    p.plan.check_chain()
    rec['chain_state'] = list(p.plan.chain_state())        # the frame plan's: the flow-only plan runs no body
    rec['band_ok'] = fp.band_ok() and p.band_ok()
    rec['finite'] = bool(torch.isfinite(flows).all().item() and all(torch.isfinite(o).all().item() for o in outs))
    rec['payload_words'] = payload_words(flows) + sum(payload_words(o) for o in outs)
    rec['repeat_equal'] = bool(torch.equal(flows.view(torch.int32), again.view(torch.int32)))
    rec['digest'] = digest(flows, *outs)
    fe, ee = [], []
    with torch.no_grad():
        for j in range(k):
            ref, parts = O.frnet_step(sd, clip[j + 1:j + 2].cpu(), clip[j:j + 1].cpu(), hp.cpu(), s, c.degradation, return_parts=True)
            ee.append(err(outs[j], ref))
            fe.append(err(flows[j:j + 1], parts['lr_flow']))
    rec['frame_err'], rec['flow_err'] = ee, fe
    if k == 1:
        o = fresh_out(1, 3, s * h, s * w)
        step(p, clip[1:2], clip[0:1], hp, o)
        torch.cuda.synchronize()
        rec['phases_equal'] = {'step': bool(torch.equal(o.view(torch.int32), outs[0].view(torch.int32)))}
    return rec


def check_record(c, rec):
    print('%-28s %6.2f s  frame %s  flow %s  body %s' % (
        c.name, rec['wall_s'], ' '.join('%.2e' % e for e in rec.get('frame_err', [])),
        ' '.join('%.2e' % e for e in rec.get('flow_err', [])), rec['chain_state']))
    print('    launches: ' + ', '.join('%s=%d' % kv for kv in rec['stats'].items() if kv[1]))
    print('    digest: ' + rec['digest'])
    got = {k: rec['stats'][k] for k in c.expect}
    assert got == c.expect, (c.name, 'launch kinds', got, c.expect)
    body = c.extra['frame_body'] if c.extra.get('fnet_only') else c.extra['body']
    assert rec['chain_state'] == [0, body in ('resident', 'chain')], (c.name, rec['chain_state'])
    assert rec['finite'] and rec['payload_words'] == 0, (c.name, 'scratch read before it was written, or output not written',
                                                        rec['finite'], rec['payload_words'])
    assert rec['band_ok'], (c.name, 'a launch wrote behind tg_frnet_workspace_floats')
    assert rec['repeat_equal'], (c.name, 'the second step on the used workspace differs from the first')
    if 'u8_mismatches' in rec:
        assert rec['u8_mismatches'] == 0, (c.name, rec['u8_mismatches'])
    if c.precision == 'fp32':
        assert max(rec['frame_err']) <= M.FRAME_TOL, (c.name, rec['frame_err'])
        assert max(rec['flow_err']) <= M.FLOW_TOL, (c.name, rec['flow_err'])
    if c.extra.get('phases') or c.extra.get('fnet_only') == 1:
        assert all(rec['phases_equal'].values()), (c.name, rec['phases_equal'])


# ---- groups -----------------------------------------------------------------------------------------------------------------
def child_main(names):
    """In a child process whose environment holds the group's switches: one JSON line per case."""
    failed = None
    for name in names:
        if failed:                       # nothing more is started on the GPU behind a case that raised
            rec = dict(name=name, error='not run: %s of the same group raised' % failed)
        else:
            try:
                rec = run_case(M.BY_NAME[name])
            except Exception as e:       # the parent reports it under the case's name
                rec, failed = dict(name=name, error='%s: %s' % (type(e).__name__, e)), name
        print(MARK + json.dumps(rec), flush=True)


def _text(s):
    return s.decode(errors='replace') if isinstance(s, bytes) else (s or '')


def run_group_in_child(key, cases):
    """({case name: record} of the cases the child reported, None or what went wrong with the child).  The child runs
    ONCE: whatever it left unreported stays unreported."""
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(dict(key))
    script = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
              "from tests.test_hip_plan_matrix import child_main\n"
              "child_main(sys.argv[1:])\n" % (ROOT_DIR, GOLDEN_DIR))
    try:
        r = subprocess.run([sys.executable, '-c', script] + [c.name for c in cases], env=env, capture_output=True,
                           text=True, timeout=600)
        out, errout, trouble = r.stdout, r.stderr, None if r.returncode == 0 else 'ended with status %d' % r.returncode
    except subprocess.TimeoutExpired as e:
        out, errout, trouble = _text(e.stdout), _text(e.stderr), 'was killed at its time limit of %d s' % e.timeout
    recs = {}
    for line in out.splitlines():
        if line.startswith(MARK):
            try:
                d = json.loads(line[len(MARK):])
            except ValueError:               # (a line cut short by the kill)
                continue
            recs[d['name']] = d
    bad = [d['name'] for d in recs.values() if 'error' in d]
    if not trouble and bad:
        trouble = 'reported that %s raised (%s)' % (bad[0], recs[bad[0]]['error'])
    if not trouble and len(recs) != len(cases):
        trouble = 'reported %d of %d cases' % (len(recs), len(cases))
    if trouble:
        trouble = 'the child of %s %s\n%s\n%s' % (dict(key), trouble, out[-2000:], errout[-4000:])
    return recs, trouble


@pytest.fixture(scope='module')
def records():
    """{case name: record}; a group's child runs when its first case is asked for, and runs once.

    Once a child has ended by a signal, at its time limit or with a non-zero status, has left a case unreported or
    reported that one raised, or a case has raised in this process, NOTHING more is started on the GPU from here: every
    case without a record by then fails as 'not run', the rest of a failed group and all later groups included."""
    done, stopped = {}, []

    def get(c):
        if c.name not in done:
            if stopped:
                pytest.fail('not run: ' + stopped[0], pytrace=False)
            key = M.env_key(c.env)
            if not key and not any(k in os.environ for k in SWITCHES):
                try:
                    done[c.name] = run_case(c)
                except BaseException as e:
                    stopped.append('%s raised in this process (%s: %s)' % (c.name, type(e).__name__, e))
                    raise
            else:
                recs, trouble = run_group_in_child(key, M.groups()[key])
                done.update(recs)
                if trouble:
                    stopped.append(trouble)
                if c.name not in done:
                    pytest.fail('not run: ' + trouble, pytrace=False)
        return done[c.name]
    yield get
    path = os.environ.get('TG_PLAN_MATRIX_JSON')
    if path:
        keep = ('stats', 'chain_state', 'frame_err', 'flow_err', 'wall_s', 'workspace_floats', 'digest')
        rows = {}
        for c in M.CASES:
            if c.name in done and 'error' not in done[c.name]:
                r = {k: done[c.name][k] for k in keep if k in done[c.name]}
                r['stats'] = {k: v for k, v in r['stats'].items() if v}
                r['env'] = c.env
                rows[c.name] = r
        with open(path, 'w') as f:
            json.dump(dict(frame_tol=M.FRAME_TOL, flow_tol=M.FLOW_TOL, cases=rows), f, indent=1)
            f.write('\n')


@pytest.mark.parametrize('case', M.CASES, ids=lambda c: c.name)
def test_plan_matrix(case, records):
    rec = records(case)
    assert 'error' not in rec, (case.name, rec.get('error'))
    check_record(case, rec)
