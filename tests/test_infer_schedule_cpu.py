"""The launch order infer_sequence(pipeline=True) and infer_stream share (frnet_infer.enqueue_batch), driven with a
recording fake (no GPU): a `lib` whose three entry points append (name, args), streams and events whose wait_event /
record append too, plain integers for device addresses."""
from types import SimpleNamespace

import pytest

import tecogan_pytorch_amd  # noqa: F401
from tecogan_pytorch_amd.models.networks import frnet_infer as F

PLAN = SimpleNamespace(handle=7000)
BASE, STRIDE = 1 << 20, 1000                # the LR frame before the batch, bytes from one LR frame to the next
HR = (50000, 60000)
U8, U8_STRIDE = 1 << 24, 300
ZFLOW, FLOW0, FLOW_BYTES = 4242, 1 << 28, 64


class Stream:
    def __init__(self, name, trace):
        self.name, self.cuda_stream, self.trace = name, {'main': 11, 'side': 22}[name], trace

    def wait_event(self, ev):
        self.trace.append(('wait', self.name, ev))


class Event:
    def __init__(self, name, trace):
        self.name, self.trace = name, trace

    def record(self, stream):
        self.trace.append(('record', self.name, stream.name))

    def __repr__(self):
        return self.name


class Lib:
    def __init__(self, trace, status=None):
        self.trace, self.status = trace, status or {}       # status: entry point -> what it returns (default 0 = TG_OK)

    def tg_frnet_step_srnet(self, *args):
        self.trace.append(('srnet', args))
        return self.status.get('srnet', 0)

    def tg_frnet_step_phase(self, *args):
        self.trace.append(('phase', args))
        return self.status.get('phase', 0)

    def tg_last_error_string(self):
        return b'injected'

    def tg_frnet_plan_flow(self, *args):
        self.trace.append(('flow', args))
        return FLOW0


class Rig:
    """One trace, and everything enqueue_batch is handed."""

    def __init__(self, status=None):
        self.trace, self.pairs = [], []
        self.lib, self.main, self.side = Lib(self.trace, status), Stream('main', self.trace), Stream('side', self.trace)

    def flow_plan(self, npair):
        self.pairs.append(npair)
        return SimpleNamespace(handle=8000 + npair)

    def event(self, name):
        return Event(name, self.trace)

    def batch(self, b, i0, cnt, lr_prev=BASE, u8=U8, ev_flow=None, ev_free=None):
        ev_flow = ev_flow if ev_flow is not None else self.event('f%d' % b)
        F.enqueue_batch(self.lib, PLAN, self.flow_plan, b, i0, cnt, lr_prev, STRIDE, HR, u8, U8_STRIDE, ZFLOW,
                        FLOW_BYTES, self.main, self.side, ev_flow, ev_free)
        return ev_flow


def srnet(flow, j, i):
    """The SRNet call of frame i of the clip, the j-th of its batch."""
    return ('srnet', (PLAN.handle, flow, BASE + (1 + j) * STRIDE, HR[i & 1], HR[(i + 1) & 1], U8 + j * U8_STRIDE, 11))


def phase(npair, slot, f0):
    return ('phase', (8000 + npair, 1, slot, BASE + (f0 + 1) * STRIDE, BASE + f0 * STRIDE, None, None, None, 22))


def test_a_lone_frame_runs_on_the_zero_flow_and_touches_nothing_else():
    rig = Rig()
    rig.batch(0, 0, 1)
    assert rig.trace == [srnet(ZFLOW, 0, 0)]
    assert rig.pairs == []


def test_first_batch_frame_zero_ahead_of_the_flow_pass():
    rig = Rig()
    ev = rig.batch(0, 0, 3)
    assert rig.trace == [srnet(ZFLOW, 0, 0),
                         phase(2, 0, 1),                        # curr = base + 2 strides, prev = base + 1 stride
                         ('record', 'f0', 'side'), ('wait', 'main', ev),
                         ('flow', (8002, 0)),
                         srnet(FLOW0, 1, 1), srnet(FLOW0 + FLOW_BYTES, 2, 2)]
    assert rig.pairs == [2]


def test_later_batch_waits_for_the_batch_two_back_and_keeps_the_clip_parity():
    rig = Rig()
    free = rig.event('s0')
    ev = rig.batch(2, 5, 2, ev_free=free)
    assert rig.trace == [('wait', 'side', free),
                         phase(2, 0, 0),
                         ('record', 'f2', 'side'), ('wait', 'main', ev),
                         ('flow', (8002, 0)),
                         srnet(FLOW0, 0, 5), srnet(FLOW0 + FLOW_BYTES, 1, 6)]
    # frame 5 reads hr[1] and writes hr[0]: the parity of the index in the clip, not in the batch
    assert rig.trace[5][1][3:5] == (HR[1], HR[0])


def test_second_batch_waits_for_no_earlier_batch():
    rig = Rig()
    ev = rig.batch(1, 3, 2, ev_free=rig.event('never'))
    assert [e for e in rig.trace if e[0] == 'wait'] == [('wait', 'main', ev)]
    assert rig.trace[0] == phase(2, 1, 0)


@pytest.mark.parametrize('entry,trace_len', [('srnet', 1), ('phase', 2)])
def test_a_failed_call_raises_before_anything_later_is_enqueued(monkeypatch, entry, trace_len):
    """Statuses go through _lib.check, which asks the loaded library for the message: the fake stands in there too."""
    from tecogan_pytorch_amd import _lib
    rig = Rig({entry: 3})
    monkeypatch.setattr(_lib, 'lib', lambda: rig.lib)
    with pytest.raises(_lib.TecoganHipError, match='injected'):
        rig.batch(0, 0, 3)
    # frame 0 failed: no flow pass; the flow pass failed: no event recorded, no frame behind it
    assert [e[0] for e in rig.trace] == ['srnet', 'phase'][:trace_len]


@pytest.mark.parametrize('first,later', [(9, 8), (3, 2), (2, 1)])
def test_whole_clips_over_clip_batches(first, later):
    for t in range(1, 41):
        rig = Rig()
        ev_s = []
        for b, (i0, cnt) in enumerate(F.clip_batches(t, first, later)):
            # both callers keep the clip's frames (a slot's, in the engine) one stride apart: frame i at BASE + (1 + i)
            rig.batch(b, i0, cnt, lr_prev=BASE + i0 * STRIDE, u8=U8 + i0 * U8_STRIDE,
                      ev_free=ev_s[b - 2] if b >= 2 else None)
            ev_s.append(rig.event('s%d' % b))
            rig.trace.append(('end', b))
        calls = [e[1] for e in rig.trace if e[0] == 'srnet']
        # every frame once, in order: its LR frame, its uint8 frame
        assert [a[2] for a in calls] == [BASE + (1 + i) * STRIDE for i in range(t)]
        assert [a[5] for a in calls] == [U8 + i * U8_STRIDE for i in range(t)]
        # the HR pair alternates without a break across batch borders, from the zero state in hr[0]
        assert [a[3:5] for a in calls] == [(HR[i & 1], HR[(i + 1) & 1]) for i in range(t)]
        assert calls[0][1] == ZFLOW and all(a[1] != ZFLOW for a in calls[1:])
        assert sum(rig.pairs) == t - 1
        # every flow pass of a batch b >= 2 has the wait for batch b - 2 right in front of it, on the side stream
        passes = [(k, e[1][2]) for k, e in enumerate(rig.trace) if e[0] == 'phase']
        ends = [k for k, e in enumerate(rig.trace) if e[0] == 'end']
        for k, slot in passes:
            b = sum(1 for e in ends if e < k)
            assert slot == b & 1
            if b >= 2:
                assert rig.trace[k - 1] == ('wait', 'side', ev_s[b - 2])
            else:
                assert rig.trace[k - 1][0] != 'wait'
