"""Host side of the scene-cut reset of infer_stream, no GPU: the numpy specification
(tests/scene_cut_ref.py) on the clips the GPU tests use, SceneCut's argument checks, the index shift of
VSRModel.infer_stream, the C ABI's refusals, and where enqueue_batch puts the conditional fills."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import tecogan_pytorch_amd  # noqa: F401
from tecogan_pytorch_amd import _lib as L
from tecogan_pytorch_amd.models.networks import SceneCut, frnet_infer as F
from procedural_weights import smooth_clip
from tests import scene_cut_ref as R


def two_scenes(la, lb):
    """A(la) | B(lb): two unrelated smooth scenes, the second inverted."""
    return torch.cat([smooth_clip(la, 3, 24, 40, seed=3), 1.0 - smooth_clip(lb, 3, 24, 40, seed=7)], 0)


def three_scenes():
    return torch.cat([smooth_clip(6, 3, 24, 40, seed=3), 1.0 - smooth_clip(7, 3, 24, 40, seed=7),
                      smooth_clip(9, 3, 24, 40, seed=5)], 0)


# ------------------------------------------------------------------ the specification
def test_quantisation_is_one_fused_multiply_add_then_floor_and_clamp():
    k = np.arange(256)
    assert np.array_equal(R.quant255((k / 255.0).astype(np.float32)), k)
    x = np.array([-0.3, 1.7, np.nan, np.inf, -np.inf, 0.0, 1.0, 0.5 / 255, 254.5 / 255], np.float32)
    q = R.quant255(x)
    assert list(q[:7]) == [0, 255, 0, 255, 0, 0, 255]
    # the fp32 value next to a boundary (k + 0.5) / 255: the exact sum is within 2^-24 relative of k + 1, and the ONE
    # rounding takes it there whichever side it lies on
    b = ((k[:255] + 0.5) / 255.0).astype(np.float32)
    assert np.array_equal(R.quant255(b), k[:255] + 1)
    assert R.luma(np.ones((3, 2, 2), np.float32)).tolist() == [[255, 255], [255, 255]]
    assert R.luma(np.zeros((3, 1, 1), np.float32)).tolist() == [[0]]


def test_statistics_of_a_hand_made_pair():
    a = np.zeros((3, 2, 4), np.float32)                      # luma 0 everywhere: bin 0
    b = np.zeros((3, 2, 4), np.float32)
    b[:, 0, :] = 1.0                                         # the top row 255: bin 31
    sad, hd = R.stats(np.stack([a, b, b]))
    assert sad.tolist() == [4 * 255, 0] and hd.tolist() == [8, 0]
    f, s, d = R.flags(np.stack([a, b, b]), 4 * 255, 8)
    assert f.tolist() == [1, 0] and s.dtype == np.uint64 and d.dtype == np.uint32
    assert R.flags(np.stack([a, b, b]), 4 * 255 + 1, 8)[0].tolist() == [0, 0]
    assert R.flags(np.stack([a, b, b]), 4 * 255, 9)[0].tolist() == [0, 0]
    assert R.flags(np.stack([a, b, b]), 0, 0, detect=False)[0].tolist() == [0, 0]
    assert R.flags(np.stack([a, b, b]), 10 ** 9, 0, forced=[0, 1], detect=True)[0].tolist() == [0, 1]
    assert R.thresholds(24.0, 0.25, 24, 40) == (23040, 480) and R.thresholds(0.1, 0.3, 1, 3) == (1, 2)


@pytest.mark.parametrize('la,lb', [(8, 18), (5, 12)])
def test_two_scenes_cut_where_they_join_and_nowhere_else(la, lb):
    cuts, scores = R.stream_cuts(two_scenes(la, lb).numpy())
    assert cuts == [la]
    assert scores[la][0] >= 60 and scores[la][1] >= 0.35           # far above the defaults, 24 and 0.25 ...
    rest = [s for i, s in enumerate(scores) if i not in (0, la)]
    assert max(s[0] for s in rest) <= 14.6 and max(s[1] for s in rest) <= 0.133      # ... and every other pair far below


def test_three_scenes():
    cuts, scores = R.stream_cuts(three_scenes().numpy())
    assert cuts == [6, 13]
    assert abs(scores[6][0] - 74.8) < 0.1 and abs(scores[6][1] - 0.345) < 0.001
    assert abs(scores[13][0] - 42.3) < 0.1 and abs(scores[13][1] - 0.38) < 0.005
    assert R.stream_cuts(three_scenes().numpy(), detect=False, at=[0, 4, 21, 22, 99])[0] == [4, 21]


# ------------------------------------------------------------------ SceneCut
def test_scene_cut_arguments():
    sc = SceneCut()
    assert (sc.mad, sc.hist, sc.detect, sc.keep_scores, sc.at, sc.cuts, sc.scores) == (24.0, 0.25, True, False,
                                                                                      frozenset(), [], [])
    assert SceneCut(at=[np.int64(3), 5]).at == {3, 5} and SceneCut(mad=0, hist=np.float32(0.5)).hist == 0.5
    for kw in ({'mad': -1.0}, {'hist': -0.1}, {'mad': float('nan')}, {'hist': float('inf')}, {'mad': '24'},
               {'mad': True}, {'at': [1.5]}, {'at': ['3']}, {'at': [True]}, {'at': 3}, {'detect': 1},
               {'keep_scores': 'yes'}):
        with pytest.raises(ValueError, match='SceneCut'):
            SceneCut(**kw)
    assert sc.thresholds(24, 40) == R.thresholds(24.0, 0.25, 24, 40)
    assert SceneCut(mad=0.1, hist=0.3).thresholds(1, 3) == (1, 2)
    assert SceneCut(at=[0, 9, 11, 17]).forced(9, 8).tolist() == [1, 0, 1, 0, 0, 0, 0, 0]
    assert SceneCut(at=[0, 2]).forced(0, 3).tolist() == [0, 0, 1]            # frame 0 is never a cut
    assert 'mad=24.0' in repr(sc)


def test_report_collects_cuts_and_scores_per_retired_batch():
    sc = SceneCut(keep_scores=True)
    sc.report(0, [0, 0, 1], [960, 0, 96000], [1920, 0, 960], 960)
    sc.report(3, [1, 0], [9600, 0], [0, 192], 960)
    assert sc.cuts == [2, 3]
    assert sc.scores == [(1.0, 1.0), (0.0, 0.0), (100.0, 0.5), (10.0, 0.0), (0.0, 0.1)]
    quiet = SceneCut()
    quiet.report(0, [0, 1], [0, 0], [0, 0], 960)
    assert quiet.cuts == [1] and quiet.scores == []


def test_engine_refuses_a_bad_scene_cut_before_anything_is_enqueued():
    from tecogan_pytorch_amd.models.networks.stream import _StreamEngine
    net = SimpleNamespace(in_nc=1, scale=4)
    with pytest.raises(ValueError, match='in_nc = 3'):
        _StreamEngine(net, iter([]), 'cpu', 'rerun', None, SceneCut())
    with pytest.raises(ValueError, match='SceneCut or None'):
        _StreamEngine(SimpleNamespace(in_nc=3, scale=4), iter([]), 'cpu', 'rerun', None, {'mad': 24.0})


# ------------------------------------------------------------------ VSRModel.infer_stream: the shift by num_pad_front
def test_shift_by_the_front_padding_in_and_out():
    outer = SceneCut(mad=20.0, hist=0.5, detect=False, at=[0, 3, 11], keep_scores=True)
    inner = outer.shifted(5)
    assert (inner.mad, inner.hist, inner.detect, inner.keep_scores) == (20.0, 0.5, False, True)
    assert inner.at == {8, 16}                                   # the caller's frame 0 is never a cut
    # the engine reports in the padded numbering: one found inside the prefix (2), one on the caller's frame 3, ...
    inner.report(0, [0, 0, 1, 0, 0, 0, 0, 0, 1], range(9), range(9), 1)
    seen = outer.absorb(inner, 5, (0, 0))
    assert seen == (2, 9) and outer.cuts == [3]
    assert outer.scores == [(float(i), i / 2) for i in range(5, 9)]
    inner.report(9, [0] * 7 + [1], range(9, 17), range(9, 17), 1)
    seen = outer.absorb(inner, 5, seen)
    assert seen == (3, 17) and outer.cuts == [3, 11] and len(outer.scores) == 12
    assert outer.absorb(inner, 5, seen) == seen and outer.cuts == [3, 11]


def test_vsr_model_infer_stream_shifts_forced_and_found_cuts(monkeypatch):
    """num_pad_front = 5 around a fake generator that records the SceneCut it is given and reports cuts in ITS numbering:
    forced and found ones, inside the padded prefix and after it."""
    from tecogan_pytorch_amd.models.vsr_model import VSRModel
    seen = {}

    class Net:
        in_nc = 3

        def eval(self):
            pass

        def infer_stream(self, frames, device, yuv=None, scene_cut=None):
            seen['sc'], seen['n'] = scene_cut, 0

            def run():
                clip = torch.cat([x if x.dim() == 4 else x.unsqueeze(0) for x in frames], 0)
                seen['n'] = len(clip)
                found = {2, 4, 9}                                    # two inside the prefix, one at the caller's 4
                for a in range(0, len(clip), 4):
                    b = min(a + 4, len(clip))
                    if scene_cut is None:
                        yield np.zeros((b - a, 8, 8, 3), np.uint8)
                        continue
                    flags = [1 if i > 0 and (i in found or i in scene_cut.at) else 0 for i in range(a, b)]
                    scene_cut.report(a, flags, [7 * i for i in range(a, b)], [2 * i for i in range(a, b)], 1)
                    yield np.zeros((b - a, 8, 8, 3), np.uint8) + np.arange(a, b, dtype=np.uint8)[:, None, None, None]
            return run()
    model = VSRModel.__new__(VSRModel)
    model.opt = {'test': {'padding_mode': 'reflect', 'num_pad_front': 5}}
    model.net_G, model.device = Net(), 'cpu'
    sc = SceneCut(at=[0, 2, 7], keep_scores=True)
    sc.cuts.append(99)                                               # a new stream starts the lists afresh
    clip = smooth_clip(10, 3, 8, 8, seed=1)
    got, upto = [], []
    for chunk in model.infer_stream((f for f in clip), scene_cut=sc):
        got.append(chunk.copy())
        upto.append((sum(len(c) for c in got), list(sc.cuts)))
    out = np.concatenate(got, 0)
    assert seen['n'] == 15 and out[:, 0, 0, 0].tolist() == list(range(5, 15))
    assert seen['sc'] is not sc and seen['sc'].at == {7, 12}         # 0 dropped, 2 and 7 moved by 5
    assert seen['sc'].cuts == [2, 4, 7, 9, 12]
    assert sc.cuts == [2, 4, 7]                                      # 2 and 4 of the padded stream fell in the prefix
    assert sc.scores == [(7.0 * i, 1.0 * i) for i in range(5, 15)]
    # once a chunk covering the caller's frames [a, b) has arrived, every cut < b is in the list
    for b, cuts in upto:
        assert [c for c in sc.cuts if c < b] == [c for c in cuts if c < b]
    # without the option the generator is called exactly as before
    list(model.infer_stream(f for f in clip))
    assert seen['sc'] is None


# ------------------------------------------------------------------ the C ABI refuses, nothing is launched
def test_abi_refusals_are_error_codes():
    lib = L.lib()
    wsb = lib.tg_scene_cut_workspace_bytes
    assert wsb(0) == 0 and wsb(-3) == 0 and wsb(1) == 8 + 2 * 32 * 4 and wsb(9) == 9 * 8 + 10 * 32 * 4
    p = 4096                                                     # any aligned non-null address: nothing is dereferenced
    ok = dict(frames=p, n=2, h=4, w=4, s_min=1, d_min=1, forced=None, detect=1, flags=p, sad=p, hdist=p, ws=p,
              wsb=wsb(2), stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.tg_scene_cut_flags(a['frames'], a['n'], a['h'], a['w'], a['s_min'], a['d_min'], a['forced'],
                                      a['detect'], a['flags'], a['sad'], a['hdist'], a['ws'], a['wsb'], a['stream'])
    for name in ('frames', 'flags', 'sad', 'hdist', 'ws'):
        assert call(**{name: None}) == -2 and b'null' in lib.tg_last_error_string()
    assert call(n=0) == -2 and call(h=0) == -2 and call(w=-1) == -2
    assert call(wsb=wsb(2) - 1) == -2 and b'workspace' in lib.tg_last_error_string()
    assert call(ws=p + 4) == -2 and call(frames=p + 2) == -2 and call(sad=p + 4) == -2
    assert call(h=1 << 15, w=(1 << 13) + 1) == -1                # more than 2^28 pixels: TG_E_SHAPE
    z = lib.tg_zero_if_flag
    assert z(None, 16, p, None) == -2 and z(p, 16, None, None) == -2
    assert z(p, -1, p, None) == -2 and z(p, 16, p + 2, None) == -2
    assert z(p, 0, p, None) == 0                                 # nothing to fill: no launch


# ------------------------------------------------------------------ enqueue_batch: where the fills go
PLAN = SimpleNamespace(handle=7000)
BASE, STRIDE = 1 << 20, 1000
HR, HR_BYTES = (50000, 60000), 4608
U8, U8_STRIDE = 1 << 24, 300
ZFLOW, FLOW0, FLOW_BYTES = 4242, 1 << 28, 64
FLAGS = 1 << 30                                                  # batch b's flags at FLAGS + 64 b


class Stream:
    def __init__(self, name, trace):
        self.name, self.cuda_stream, self.trace = name, {'main': 11, 'side': 22}[name], trace

    def wait_event(self, ev):
        self.trace.append(('wait', self.name))


class Event:
    def __init__(self, trace):
        self.trace = trace

    def record(self, stream):
        self.trace.append(('record', stream.name))


class Lib:
    def __init__(self, trace, status=None):
        self.trace, self.status = trace, status or {}

    def tg_frnet_step_srnet(self, *args):
        self.trace.append(('srnet', args))
        return self.status.get('srnet', 0)

    def tg_frnet_step_phase(self, *args):
        self.trace.append(('phase', args))
        return 0

    def tg_zero_if_flag(self, *args):
        self.trace.append(('fill', args))
        return self.status.get('fill', 0)

    def tg_last_error_string(self):
        return b'injected'

    def tg_frnet_plan_flow(self, *args):
        return FLOW0


def run_clip(t, first, later, with_reset, status=None):
    trace = []
    lib, main, side = Lib(trace, status), Stream('main', trace), Stream('side', trace)
    for b, (i0, cnt) in enumerate(F.clip_batches(t, first, later)):
        kw = {'reset': (FLAGS + 64 * b, HR_BYTES)} if with_reset else {}
        F.enqueue_batch(lib, PLAN, lambda npair: SimpleNamespace(handle=8000 + npair), b, i0, cnt, BASE + i0 * STRIDE,
                        STRIDE, HR, U8 + i0 * U8_STRIDE, U8_STRIDE, ZFLOW, FLOW_BYTES, main, side, Event(trace),
                        Event(trace) if b >= 2 else None, **kw)
        trace.append(('end', b, i0))
    return trace


@pytest.mark.parametrize('first,later', [(9, 8), (3, 2), (2, 1)])
def test_one_fill_directly_before_every_srnet_call_but_the_first(first, later):
    for t in range(1, 41):
        plain, trace = run_clip(t, first, later, False), run_clip(t, first, later, True)
        # without `reset`: today's calls; with it: the same calls plus the fills
        assert not any(e[0] == 'fill' for e in plain)
        assert [e for e in trace if e[0] != 'fill'] == plain
        fills = [k for k, e in enumerate(trace) if e[0] == 'fill']
        steps = [k for k, e in enumerate(trace) if e[0] == 'srnet']
        assert len(steps) == t and [k + 1 for k in fills] == steps[1:]
        assert steps[0] == 0 and trace[0][1][1] == ZFLOW              # the stream's frame 0: no fill, the zero flow
        starts = [e[2] for e in trace if e[0] == 'end']
        for i, k in enumerate(steps[1:], start=1):
            b = sum(1 for e in trace[:k] if e[0] == 'end')
            j = i - starts[b]
            # on the state frame i reads, at the flag of frame j of batch b, on the main stream
            assert trace[k - 1][1] == (HR[i & 1], HR_BYTES, FLAGS + 64 * b + 4 * j, 11)
            assert trace[k][1][3] == HR[i & 1]


def test_a_failed_fill_raises_before_the_srnet_call_behind_it(monkeypatch):
    trace = []
    fake = Lib(trace, {'fill': 3})
    monkeypatch.setattr(L, 'lib', lambda: fake)
    with pytest.raises(L.TecoganHipError, match='tg_zero_if_flag.*injected'):
        F.enqueue_batch(fake, PLAN, lambda npair: SimpleNamespace(handle=8000 + npair), 0, 0, 3, BASE, STRIDE, HR, U8,
                        U8_STRIDE, ZFLOW, FLOW_BYTES, Stream('main', trace), Stream('side', trace), Event(trace), None,
                        reset=(FLAGS, HR_BYTES))
    assert [e[0] for e in trace] == ['srnet', 'phase', 'record', 'wait', 'fill']


def test_parse_args_takes_the_scene_cut_options():
    from tecogan_pytorch_amd import main as M
    a = M.parse_args(['--mode', 'infer', '--input', 'x', '--output', 'y'])
    assert a.scene_cut is False and M.scene_cut_option(a) is None
    a = M.parse_args(['--mode', 'infer', '--input', 'x', '--output', 'y', '--scene-cut', '--scene-cut-mad', '30',
                      '--scene-cut-hist', '0.4'])
    sc = M.scene_cut_option(a)
    assert isinstance(sc, SceneCut) and (sc.mad, sc.hist, sc.detect, sc.at) == (30.0, 0.4, True, frozenset())
