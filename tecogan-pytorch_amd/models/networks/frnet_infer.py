"""What FRNet.infer_sequence and FRNet.infer_stream share, and what neither a network nor the stream engine owns: the
device plan behind tg_frnet_step*, the long-lived side streams, the batch partition of a clip, and the ONE place that
enqueues a batch's launches (enqueue_batch).  Uses a network only through its attributes."""
import ctypes
import os

import torch

from ... import _lib as L
from .. import packs


def _norm_device(device):
    """'cuda' -> cuda:<current>: plans and side streams are cached per device, and torch.device('cuda')
    != torch.device('cuda', 0) -- rounds 1-2 re-created the side stream on every clip because of it."""
    dev = torch.device(device)
    if dev.type == 'cuda' and dev.index is None:
        dev = torch.device('cuda', torch.cuda.current_device())
    return dev


_SIDE_STREAMS = {}


def side_stream(dev, kind='side'):
    """ONE long-lived side stream per (device, kind) for the whole process.  Handing out a new pool
    stream per clip (what rounds 1-2 did by accident) walks torch's stream pool across the runtime's
    four hardware queues, so every few clips the side stream shares the main stream's queue and the
    overlap is silently lost; a stable stream was measured at the full two-stream rate with and
    without DEBUG_HIP_DYNAMIC_QUEUES, with HIP initialised before or after the import, and next
    to an RCCL process group (tools/stream_probe.py).  A stream created with a
    CU mask (a hardware queue of its own) and a high-priority stream were measured WORSE."""
    key = (str(_norm_device(dev)), kind)
    st = _SIDE_STREAMS.get(key)
    if st is None:
        st = _SIDE_STREAMS[key] = torch.cuda.Stream(device=_norm_device(dev))
    return st


class _StepPlan:
    """Caller-owned device state behind one tg_frnet_plan: packed weights,
    workspace, and the opaque plan handle."""

    def __init__(self, net, n, h, w, device, fnet_only=False, precision='fp32'):
        lib = L.lib()
        self.cfg = L.FrnetCfg(net.in_nc, net.out_nc, net.nf, net.nb, net.scale,
                              net.srnet.up_mode(), n, h, w, 1 if fnet_only else 0)
        self.n, self.fh, self.fw = n, h // 8 * 8, w // 8 * 8
        nfl = lib.tg_frnet_workspace_floats(ctypes.byref(self.cfg))
        if nfl == 0:
            raise L.TecoganHipError(f'tg_frnet_workspace_floats: unsupported config '
                                    f'n={n} h={h} w={w} nf={net.nf} scale={net.scale}')
        self.workspace = torch.empty(nfl, dtype=torch.float32, device=device)
        self.keep = []          # packed tensors must outlive the plan
        layers = net.fnet.layers() + net.srnet.layers()
        first_up = net.srnet.conv_up['0'] if hasattr(net.srnet, 'conv_up') and '0' in net.srnet.conv_up else None
        arr = (L.LayerWeights * len(layers))()
        for i, m in enumerate(layers):
            if m.cout <= 4:      # direct small-cout kernel takes plain OIHW
                wt = m.weight.detach().contiguous()
            else:
                wt, _ = m.packed()
            b = m.bias.detach().contiguous()
            u = m.packed_wino() if m.cout > 4 else None
            if m is first_up and not fnet_only and net.scale == 4 and net.nf == 64 and n == 1 and \
                    os.environ.get('TG_WINO_RES_CT', '1') != '0':
                # SRNet's first up-sampling layer as the tail of the resident body launch (tg_conv3x3_wino_res.hip);
                # the plan uses it when the frame runs that launch.  TG_WINO_RES_CT=0: always a launch of its own.
                u = packs.get(m, 'wres_convt')
            self.keep += [wt, b, u]
            arr[i].w, arr[i].b = wt.data_ptr(), b.data_ptr()
            arr[i].u = u.data_ptr() if u is not None else None
        self.handle = ctypes.c_void_p()
        L.check(lib.tg_frnet_plan_create(ctypes.byref(self.cfg), arr, len(layers),
                                         self.workspace.data_ptr(), ctypes.byref(self.handle)),
                'tg_frnet_plan_create')
        self.precision = 'fp32'
        if precision == 'fp16' and not fnet_only:
            # fp16 SRNet body: the plan packs fp16 weights from the plain tensors, once
            nws = lib.tg_frnet_f16_workspace_bytes(ctypes.byref(self.cfg))
            if nws == 0:
                raise L.TecoganHipError(f"precision='fp16' needs nf = 64 (nf={net.nf}); there is no fp32 fallback")
            self.workspace_f16 = torch.empty(nws, dtype=torch.uint8, device=device)
            body = net.srnet.layers()[:2 + 2 * net.nb]         # conv_in, block convs, first up-sampling layer
            plain = (L.LayerWeights * len(body))()
            for i, m in enumerate(body):
                wt, b = m.weight.detach().contiguous(), m.bias.detach().contiguous()
                self.keep += [wt, b]
                plain[i].w, plain[i].b, plain[i].u = wt.data_ptr(), b.data_ptr(), None
            L.check(lib.tg_frnet_plan_set_precision(self.handle, L.PREC_F16, plain, len(body),
                                                    self.workspace_f16.data_ptr()), 'tg_frnet_plan_set_precision')
            self.precision = 'fp16'

    def check_chain(self):
        """Raise if a workgroup of the chained SRNet launch gave up waiting for a producer tile since
        the last check (tg_frnet_plan_chain_status; the frames enqueued on this plan since then were
        built on stale data).  A host read of a pinned counter -- no synchronisation; after a
        synchronisation it covers everything enqueued so far.  Every tg_frnet_step* call makes the
        same check on entry, so a fault also surfaces on the NEXT call of any kind on this plan;
        the plan then runs one launch per layer until it re-arms (set_chain_rearm: after 64 clean frames by default,
        the wait doubling with every fault of a re-armed body)."""
        L.check(L.lib().tg_frnet_plan_chain_status(self.handle, None, None), 'chained SRNet launch')

    def chain_state(self):
        """(faults reported so far, chained launch still in use)."""
        f, a = ctypes.c_int(0), ctypes.c_int(0)
        L.lib().tg_frnet_plan_chain_status(self.handle, ctypes.byref(f), ctypes.byref(a))
        return f.value, bool(a.value)

    def set_chain_rearm(self, first_after_frames):
        """Frames on the per-layer fallback before a faulted one-launch body is tried again (0: never; default 64,
        doubled by every fault of a re-armed body) -- tg_frnet_plan_set_chain_rearm."""
        L.check(L.lib().tg_frnet_plan_set_chain_rearm(self.handle, int(first_after_frames)), 'tg_frnet_plan_set_chain_rearm')

    def rearm_state(self):
        """(times the one-launch body was armed again, back-off in force in frames)."""
        r, w = ctypes.c_int(0), ctypes.c_int(0)
        L.check(L.lib().tg_frnet_plan_chain_rearms(self.handle, ctypes.byref(r), ctypes.byref(w)), 'tg_frnet_plan_chain_rearms')
        return r.value, w.value

    def hold_chain_rearm(self, hold):
        """While held, frames enqueued on a fallen-back plan neither count towards the back-off nor arm the one-launch
        body again (tg_frnet_plan_hold_chain_rearm): infer_stream repairs a faulted batch under it."""
        L.check(L.lib().tg_frnet_plan_hold_chain_rearm(self.handle, 1 if hold else 0), 'tg_frnet_plan_hold_chain_rearm')

    def __del__(self):
        try:
            if getattr(self, 'handle', None):
                L.lib().tg_frnet_plan_destroy(self.handle)
        except Exception:
            pass


# infer_sequence / infer_stream: most frame pairs (over all clips of the call) in a clip's FIRST batched flow pass --
# frame 1 waits for that pass, so it stays short whatever TG_FNET_BATCH says (EXPERIMENTS.md, round 5)
FNET_FIRST_PASS_FRAMES = 8


def stream_batch_sizes(fnet_batch=None, k=1):
    """(frames of the first batch, frames of every later one) of infer_sequence(pipeline=True) and infer_stream, for k
    lockstep clips: the only place that reads TG_FNET_BATCH.  The partition does not depend on the clip length -- the
    first batch is the first flow pass (at most FNET_FIRST_PASS_FRAMES // k pairs) plus frame 0, which needs no flow;
    later ones are TG_FNET_BATCH // k frames; the last is whatever is left."""
    if fnet_batch is None:
        fnet_batch = int(os.environ.get('TG_FNET_BATCH', '8'))
    later = max(1, int(fnet_batch) // k)
    return max(1, min(later, max(1, FNET_FIRST_PASS_FRAMES // k))) + 1, later


def clip_batches(tot_frm, first, later):
    """[(first frame, frames)] of a clip whose length is known: `first` frames, then `later` at a time, the rest last
    (what stream_rebatch hands out piece by piece without knowing the length)."""
    batches, i0 = [], 0
    while i0 < tot_frm:
        cnt = min(later if batches else first, tot_frm - i0)
        batches.append((i0, cnt))
        i0 += cnt
    return batches


def enqueue_batch(lib, plan, flow_plan, b, i0, cnt, lr_prev, lr_stride, hr, u8, u8_stride, zflow, flow_bytes,
                  main, side, ev_flow, ev_free, *, reset=None, after=None):
    """Enqueue the launches of batch b = frames i0 .. i0 + cnt - 1 of a clip, and nothing else: the order both
    infer_sequence(pipeline=True) and infer_stream produce their frames in, which is why they agree bit for bit.

    Frame 0 warps the ZERO state (reference tecogan_nets.py:266-268): its warped frame is zero whatever the flow, so it runs on
    the all-zero flow buffer `zflow` AHEAD of the first flow pass (the GPU has work ~0.3 ms earlier; that flow is never
    estimated).  The flows of the batch's other frames come from ONE batched tg_frnet_step_phase on `side` into flow
    slot b & 1 -- free once batch b - 2 has consumed it (`ev_free`: that batch's end on `main`; None when b < 2) --
    `ev_flow` hands them over to `main`, and tg_frnet_step_srnet runs frame by frame there on the HR ping-pong pair,
    whose parity follows the frame's index in the CLIP.

    plan: the frame plan; flow_plan(npair) -> the flow-only plan of npair frame pairs (both: .handle).  Everything else
    is a device address or a byte count: lr_prev the LR frame BEFORE the batch, the batch's frames following it
    lr_stride bytes apart; hr the two HR states; u8 the batch's first uint8 frame, u8_stride bytes a frame;
    flow_bytes one frame's flows.  The caller's own business stays around the call: the waits for the batch's input,
    recording its end on `main` (a later batch's ev_free), and what happens to the uint8 frames.  Every status goes
    through _lib.check (the one thing not taken as an argument): a non-zero one raises before anything later is enqueued.

    reset = (flags_addr, hr_bytes) (infer_stream with a SceneCut): one int32 flag per frame of
    the batch in device memory.  Directly in front of the tg_frnet_step_srnet of every frame j of the batch but the
    stream's frame 0, tg_zero_if_flag(hr[i & 1], hr_bytes, flags_addr + 4 j) goes onto `main`: with the flag set the
    frame warps the zero state, as a clip's frame 0 does, whatever its flow.  None: exactly the calls above.

    after (infer_stream with a 10- or 12-bit output): a callable invoked directly behind the
    tg_frnet_step_srnet of every frame j of the batch, the stream's frame 0 included, with (j, the address of the HR
    state that launch writes); what it enqueues on `main` reads the float frame before the next one replaces its
    predecessor.  None: exactly the calls above."""
    check, step, handle, ms = L.check, lib.tg_frnet_step_srnet, plan.handle, main.cuda_stream
    lr = lr_prev + lr_stride
    if i0 == 0:
        check(step(handle, zflow, lr, hr[0], hr[1], u8, ms), 'tg_frnet_step_srnet')
        if after is not None:
            after(0, hr[1])
    f0 = 1 if i0 == 0 else 0                    # frame 0's flow is never used: not estimated
    npair = cnt - f0
    if npair <= 0:
        return
    fplan = flow_plan(npair)
    if b >= 2:
        side.wait_event(ev_free)
    check(lib.tg_frnet_step_phase(fplan.handle, 1, b & 1, lr + f0 * lr_stride, lr_prev + f0 * lr_stride,
                                  None, None, None, side.cuda_stream), 'tg_frnet_step_phase(1)')
    ev_flow.record(side)
    main.wait_event(ev_flow)
    flow0 = lib.tg_frnet_plan_flow(fplan.handle, b & 1)
    for j in range(f0, cnt):
        i = i0 + j
        if reset is not None:                   # (i > 0: the stream's frame 0 ran above, and never starts a scene)
            check(lib.tg_zero_if_flag(hr[i & 1], reset[1], reset[0] + 4 * j, ms), 'tg_zero_if_flag')
        check(step(handle, flow0 + (j - f0) * flow_bytes, lr + j * lr_stride, hr[i & 1], hr[(i + 1) & 1],
                   u8 + j * u8_stride, ms), 'tg_frnet_step_srnet')
        if after is not None:
            after(j, hr[(i + 1) & 1])
