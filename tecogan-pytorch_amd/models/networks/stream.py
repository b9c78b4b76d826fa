"""FRNet.infer_stream (DESIGN.md sections 7d, 7e, 7h, 7i): input parsing, the batch ring, the raw-video form Yuv420, the
PNG output form Png, the scene-cut option SceneCut and the engine that runs a clip of any length through rings of STREAM_SLOTS batches.  A batch's launches are frnet_infer's
enqueue_batch, the ones infer_sequence(pipeline=True) enqueues.  Uses the network only through its attributes."""
import math

import numpy as np
import torch

from ... import _lib as L
from .frnet_infer import _norm_device, enqueue_batch, stream_batch_sizes


# infer_stream: ring slots = batches enqueued and not yet handed to the caller.  While batch b is in the caller's hands
# batches b+1 and b+2 are in flight (two flow slots' worth of work, ~11 ms of GPU time at 134x320), so the input is
# never pulled more than three internal batches ahead of what has been yielded.
STREAM_SLOTS = 3


def stream_frames(item, in_nc=3):
    """One input item of infer_stream -> (kind, tensor with a leading frame axis).
    kind 'u8': (h,w,c) / (n,h,w,c) uint8 on the host (numpy or torch) -> (n,h,w,c);
    kind 'f32': (c,h,w) / (n,c,h,w) float32 in [0,1], host or device -> (n,c,h,w).
    Anything else is a ValueError."""
    x = item
    if isinstance(x, np.ndarray):
        if x.dtype not in (np.uint8, np.float32):
            raise ValueError(f'infer_stream: frames are uint8 (h,w,c) or float32 (c,h,w); got numpy {x.dtype}')
        x = torch.from_numpy(np.ascontiguousarray(x))
    if not torch.is_tensor(x):
        raise ValueError(f'infer_stream: a frame is a numpy array or a torch tensor, got {type(item).__name__}')
    if x.dim() not in (3, 4):
        raise ValueError(f'infer_stream: a frame has 3 axes and a chunk of frames 4; got shape {tuple(x.shape)}')
    if x.dim() == 3:
        x = x.unsqueeze(0)
    if x.dtype == torch.uint8:
        if x.is_cuda:
            raise ValueError('infer_stream: uint8 frames are taken from the host (they go up as bytes)')
        if x.shape[3] != in_nc:
            raise ValueError(f'infer_stream: uint8 frames are (h,w,{in_nc}); got shape {tuple(x.shape[1:])}')
        return 'u8', x
    if x.dtype == torch.float32:
        if x.shape[1] != in_nc:
            raise ValueError(f'infer_stream: float32 frames are ({in_nc},h,w); got shape {tuple(x.shape[1:])}')
        return 'f32', x
    raise ValueError(f'infer_stream: frames are uint8 (h,w,c) or float32 (c,h,w); got {x.dtype}')


class StreamFormat:
    """Form of a stream's frames, fixed by its first item: kind, size, and host or device.  check() refuses an item
    of another form or size (ValueError) before any frame of it is taken."""

    def __init__(self, kind, x):
        self.kind, self.cuda = kind, bool(x.is_cuda)
        self.h, self.w = (x.shape[1], x.shape[2]) if kind == 'u8' else (x.shape[2], x.shape[3])

    def check(self, kind, x):
        h, w = (x.shape[1], x.shape[2]) if kind == 'u8' else (x.shape[2], x.shape[3])
        if (h, w) != (self.h, self.w):
            raise ValueError(f'infer_stream: frame size changed mid-stream: {h}x{w} after {self.h}x{self.w}')
        if kind != self.kind or bool(x.is_cuda) != self.cuda:
            raise ValueError('infer_stream: every item of a stream has the form of the first '
                             f"({self.kind}, {'device' if self.cuda else 'host'})")


def stream_frames_yuv(item, yuv):
    """One input item of a yuv stream -> (n, frame_bytes) uint8 host tensor: a 1-D item is one I420 frame, a 2-D item
    a chunk of frames.  Anything else is a ValueError."""
    x = item
    if isinstance(x, np.ndarray):
        if x.dtype != np.uint8:
            raise ValueError(f'infer_stream: I420 frames are uint8; got numpy {x.dtype}')
        x = torch.from_numpy(np.ascontiguousarray(x))
    if not torch.is_tensor(x):
        raise ValueError(f'infer_stream: a frame is a numpy array or a torch tensor, got {type(item).__name__}')
    if x.dtype != torch.uint8:
        raise ValueError(f'infer_stream: I420 frames are uint8; got {x.dtype}')
    if x.is_cuda:
        raise ValueError('infer_stream: I420 frames are taken from the host (they go up as bytes)')
    if x.dim() not in (1, 2) or x.shape[-1] != yuv.frame_bytes:
        raise ValueError(f'infer_stream: an I420 frame of {yuv.h}x{yuv.w} is ({yuv.frame_bytes},) and a chunk '
                         f'(n, {yuv.frame_bytes}); got shape {tuple(x.shape)}')
    return x.unsqueeze(0) if x.dim() == 1 else x


def stream_parts(frames, in_nc=3, yuv=None):
    """Lazily: (kind, tensor (n, ...)) for every non-empty item of `frames`, each checked against the first.
    yuv (a Yuv420): the items are I420 frames / chunks, kind 'yuv', each checked against the spec."""
    if yuv is not None:
        for item in frames:
            x = stream_frames_yuv(item, yuv)
            if x.shape[0]:
                yield 'yuv', x
        return
    fmt = None
    for item in frames:
        kind, x = stream_frames(item, in_nc)
        if fmt is None:
            fmt = StreamFormat(kind, x)
        else:
            fmt.check(kind, x)
        if x.shape[0]:
            yield kind, x


def stream_rebatch(parts, first, later):
    """Cut a lazy sequence of (kind, tensor (n, ...)) parts into the engine's batches WITHOUT knowing the length: yields
    (batch index, offset inside the batch, piece, batch full) piece by piece, and pulls the next part only when the
    previous one has been handed out entirely.  The last batch is whatever has been handed out when the input ends."""
    b, fill, size = 0, 0, first
    for _, x in parts:
        pos, n = 0, x.shape[0]
        while pos < n:
            m = min(size - fill, n - pos)
            piece, off = x[pos:pos + m], fill
            pos, fill = pos + m, fill + m
            full = fill == size
            if full:
                nb, fill, size = b, 0, later
                b += 1
                yield nb, off, piece, True
            else:
                yield b, off, piece, False


class StreamRing:
    """Slot bookkeeping of infer_stream: batch b lives in slot b % slots from submit() to retire(); at most `slots`
    batches are in flight, retired in order."""

    def __init__(self, slots=STREAM_SLOTS):
        self.slots, self.inflight = slots, []       # inflight: [batch index, first frame, frames], oldest first
        self.next_batch, self.next_frame = 0, 0

    def full(self):
        return len(self.inflight) >= self.slots

    def slot(self, b):
        return b % self.slots

    def submit(self, cnt):
        if self.full():
            raise RuntimeError('infer_stream: no free ring slot')
        rec = (self.next_batch, self.next_frame, cnt)
        self.inflight.append(rec)
        self.next_batch, self.next_frame = self.next_batch + 1, self.next_frame + cnt
        return rec

    def oldest(self):
        return self.inflight[0]

    def retire(self):
        return self.inflight.pop(0)


class Yuv420:
    """Raw-video form of a stream (FRNet.infer_stream(yuv=...)): planar 8-bit YUV 4:2:0 (I420)
    frames of h x w on the way in and of s*h x s*w on the way out.  matrix 'bt601' | 'bt709', full_range (bool),
    siting 'center' (y4m C420jpeg) | 'left' (y4m C420mpeg2).  Frozen."""
    __slots__ = ('h', 'w', 'matrix', 'full_range', 'siting')

    def __init__(self, h, w, matrix='bt709', full_range=False, siting='left'):
        for name, v in (('h', h), ('w', w)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 2:
                raise ValueError(f'Yuv420: {name} is an integer >= 2, got {v!r}')
        if matrix not in L.YUV_MATRIX:
            raise ValueError(f'Yuv420: matrix is one of {sorted(L.YUV_MATRIX)}, got {matrix!r}')
        if siting not in L.YUV_SITING:
            raise ValueError(f'Yuv420: siting is one of {sorted(L.YUV_SITING)}, got {siting!r}')
        if not isinstance(full_range, (bool, np.bool_)):
            raise ValueError(f'Yuv420: full_range is a bool, got {full_range!r}')
        for name, v in (('h', int(h)), ('w', int(w)), ('matrix', matrix), ('full_range', bool(full_range)),
                        ('siting', siting)):
            object.__setattr__(self, name, v)

    def __setattr__(self, name, value):
        raise AttributeError('Yuv420 is frozen')

    def __delattr__(self, name):
        raise AttributeError('Yuv420 is frozen')

    def _key(self):
        return (self.h, self.w, self.matrix, self.full_range, self.siting)

    def __eq__(self, other):
        return isinstance(other, Yuv420) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return 'Yuv420(h=%d, w=%d, matrix=%r, full_range=%r, siting=%r)' % self._key()

    @property
    def frame_bytes(self):
        return self.h * self.w + 2 * ((self.h + 1) // 2) * ((self.w + 1) // 2)

    def out_frame_bytes(self, scale):
        """Bytes of a super-resolved frame (s*h and s*w are even: the scale is 2 or 4)."""
        if scale < 1 or (scale * self.h) % 2 or (scale * self.w) % 2:
            raise ValueError(f'Yuv420: an output frame has even sides; scale {scale} gives {scale * self.h}x{scale * self.w}')
        return scale * self.h * scale * self.w * 3 // 2

    def codes(self):
        """(matrix, full_range, siting) as the C ABI takes them."""
        return L.YUV_MATRIX[self.matrix], int(self.full_range), L.YUV_SITING[self.siting]


class Png:
    """PNG output form of a stream (FRNet.infer_stream(png=...)): every super-resolved frame
    leaves the device as one complete 8-bit RGB PNG file, encoded there by tg_png_encode_u8.  filter 'adaptive' (per
    row the type with the smallest sum of |int8(byte)|) | 'none' (type 0 on every row).  Huffman-only deflate: the
    files are larger than zlib's.  Frozen."""
    __slots__ = ('filter',)

    def __init__(self, filter='adaptive'):
        if not isinstance(filter, str) or filter not in L.PNG_FILTER:
            raise ValueError(f'Png: filter is one of {sorted(L.PNG_FILTER)}, got {filter!r}')
        object.__setattr__(self, 'filter', filter)

    def __setattr__(self, name, value):
        raise AttributeError('Png is frozen')

    def __delattr__(self, name):
        raise AttributeError('Png is frozen')

    def __eq__(self, other):
        return isinstance(other, Png) and self.filter == other.filter

    def __hash__(self):
        return hash(('Png', self.filter))

    def __repr__(self):
        return 'Png(filter=%r)' % self.filter

    def code(self):
        """The filter as the C ABI takes it."""
        return L.PNG_FILTER[self.filter]


class SceneCut:
    """Scene-cut option of a stream (FRNet.infer_stream(scene_cut=...)) and the caller's handle on
    what it found.  At a cut the recurrence restarts from the zero HR state, which makes the frame the frame 0 of a clip
    of its own, bit for bit.  A frame is a cut when the mean absolute luma difference to the frame before it is at
    least `mad` (in 8-bit levels) AND the L1 distance of the two 32-bin luma histograms is at least `hist` (as a share
    of its maximum 2 h w), both in exact integers on the device; detect=False switches the detector off.  `at` forces
    cuts at these frame indices whatever the detector says.  Frame 0 of the stream is never a cut.  The defaults have
    NOT been validated on real footage; fades and dissolves are not detected, a flash resets.

    .cuts: the cut frames' indices, in the numbering of the frames the caller fed, appended when a batch is retired,
    before its chunk is yielded: once a chunk covering frames [a, b) has been received every cut < b is in the list.
    .scores (keep_scores=True): (mean absolute luma difference, histogram distance / 2 h w) per frame, for tuning the
    thresholds.  One SceneCut serves one stream at a time; a new stream clears both lists."""

    def __init__(self, mad=24.0, hist=0.25, detect=True, at=(), keep_scores=False):
        for name, v in (('mad', mad), ('hist', hist)):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or \
                    not math.isfinite(v) or v < 0:
                raise ValueError(f'SceneCut: {name} is a finite number >= 0, got {v!r}')
        for name, v in (('detect', detect), ('keep_scores', keep_scores)):
            if not isinstance(v, (bool, np.bool_)):
                raise ValueError(f'SceneCut: {name} is a bool, got {v!r}')
        try:
            at = tuple(at)
        except TypeError:
            raise ValueError(f'SceneCut: at is a sequence of frame indices, got {at!r}') from None
        for v in at:
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f'SceneCut: at holds integer frame indices, got {v!r}')
        self.mad, self.hist, self.detect, self.keep_scores = float(mad), float(hist), bool(detect), bool(keep_scores)
        self.at = frozenset(int(v) for v in at)
        self.cuts, self.scores = [], []

    def __repr__(self):
        return 'SceneCut(mad=%r, hist=%r, detect=%r, at=%r, keep_scores=%r)' % (
            self.mad, self.hist, self.detect, sorted(self.at), self.keep_scores)

    def thresholds(self, h, w):
        """(S_min, D_min) as the C ABI takes them: ceil(mad h w) and ceil(hist 2 h w)."""
        top = 2 ** 64 - 1
        return min(top, math.ceil(self.mad * h * w)), min(top, math.ceil(self.hist * 2 * h * w))

    def forced(self, i0, cnt):
        """uint8 mask of frames i0 .. i0 + cnt - 1: 1 where `at` forces a cut.  Never frame 0."""
        return np.array([1 if i > 0 and i in self.at else 0 for i in range(i0, i0 + cnt)], np.uint8)

    def report(self, i0, flags, sad, hdist, n_pixels):
        """A retired batch's results (host arrays, one entry per frame from frame i0 on) into .cuts / .scores."""
        self.cuts.extend(i0 + j for j, f in enumerate(flags) if f)
        if self.keep_scores:
            self.scores.extend((int(s) / n_pixels, int(d) / (2 * n_pixels)) for s, d in zip(sad, hdist))

    def shifted(self, n_pad):
        """The SceneCut of a stream that runs n_pad frames of padding in front of the caller's (VSRModel.infer_stream):
        the same thresholds, `at` moved by n_pad; an index below 1 (the caller's frame 0 and before) is dropped."""
        return SceneCut(self.mad, self.hist, self.detect, [a + n_pad for a in self.at if a > 0], self.keep_scores)

    def absorb(self, inner, n_pad, seen):
        """Take over what `inner` (= self.shifted(n_pad)) has reported since the last call, in the caller's numbering;
        cuts and scores of the padded prefix are dropped.  seen = (cuts, scores) taken over so far; returns the new one."""
        nc, ns = seen
        self.cuts.extend(c - n_pad for c in inner.cuts[nc:] if c >= n_pad)
        self.scores.extend(inner.scores[max(ns, n_pad):])
        return len(inner.cuts), len(inner.scores)


def yuv420_planes(chunk, H, W):
    """(Y, U, V) views of I420 frames: chunk (m, frame_bytes) -> (m,H,W), (m,ch,cw), (m,ch,cw); a single frame
    (frame_bytes,) -> (H,W), (ch,cw), (ch,cw).  numpy or torch; nothing is copied."""
    ch, cw = (H + 1) // 2, (W + 1) // 2
    if chunk.shape[-1] != H * W + 2 * ch * cw:
        raise ValueError(f'yuv420_planes: {H}x{W} frames have {H * W + 2 * ch * cw} bytes; got shape {tuple(chunk.shape)}')
    lead = tuple(chunk.shape[:-1])
    return (chunk[..., :H * W].reshape(lead + (H, W)),
            chunk[..., H * W:H * W + ch * cw].reshape(lead + (ch, cw)),
            chunk[..., H * W + ch * cw:].reshape(lead + (ch, cw)))


class _StreamEngine:
    """State of one FRNet.infer_stream (see there).  Everything the device touches is allocated once, at the first
    frame: STREAM_SLOTS slots of {LR batch + the frame before it, uint8 frames on the device, pinned uint8 frames,
    HR state snapshot, input staging, events}, and the HR ping-pong pair.  With a Yuv420 the staging and the pinned
    output hold I420 frames, and a slot has its I420 output on the device as well.  With a Png a slot has, on the device
    and pinned, one buffer of the batch's file sizes followed by one tg_png_capacity region per frame; _compute puts ONE
    tg_png_encode_u8 behind the batch's last frame, that buffer is what comes down, and the yielded views are cut from
    the pinned slot by the sizes once the download event has passed.  The encoder's workspace is one for all slots:
    every call is on the caller's stream.

    With a SceneCut a slot also has, on the device, one flag, one SAD and one histogram distance
    per frame, the forced mask and the detector's workspace, and pinned mirrors of the mask and of the results.
    _upload runs tg_scene_cut_flags on the slot's LR frames on the copy stream, behind whatever wrote them; _compute
    hands the flags' address to enqueue_batch, which puts one tg_zero_if_flag in front of every frame's SRNet launch;
    the results come down behind the frames and reach SceneCut.cuts when the batch is retired.  The host never waits
    for a decision.  The repair path needs no scene-cut code: it runs _compute again, which reads the same per-slot
    flags, and the snapshot it restores was taken before the batch's first conditional fill."""

    def __init__(self, net, frames, device, on_fault, yuv=None, scene_cut=None, png=None):
        if on_fault not in ('rerun', 'raise'):
            raise ValueError(f"on_fault must be 'rerun' or 'raise', got {on_fault!r}")
        if png is not None:
            if not isinstance(png, Png):
                raise ValueError(f'png must be a Png or None, got {type(png).__name__}')
            if yuv is not None:
                raise ValueError('infer_stream: png and yuv are two forms of the output; pass one of them')
            if net.in_nc != 3:
                raise ValueError(f'png needs RGB frames (in_nc = 3), this network has in_nc = {net.in_nc}')
        if yuv is not None:
            if not isinstance(yuv, Yuv420):
                raise ValueError(f'yuv must be a Yuv420 or None, got {type(yuv).__name__}')
            yuv.out_frame_bytes(net.scale)
        if scene_cut is not None:
            if not isinstance(scene_cut, SceneCut):
                raise ValueError(f'scene_cut must be a SceneCut or None, got {type(scene_cut).__name__}')
            if net.in_nc != 3:
                raise ValueError(f'scene_cut needs RGB frames (in_nc = 3), this network has in_nc = {net.in_nc}')
            scene_cut.cuts.clear()
            scene_cut.scores.clear()
        self.yuv, self.scene_cut, self.png = yuv, scene_cut, png
        self.net, self.frames, self.on_fault = net, frames, on_fault
        self.dev = _norm_device(device if device is not None else next(net.parameters()).device)
        self.closed, self.warned, self.reruns = False, False, 0
        self.ring = StreamRing()
        self.first, self.later = stream_batch_sizes()
        self.plan, self.pending_dl, self.prev_rec = None, None, None

    # -- allocation (once) ---------------------------------------------------------------------------------------
    def _open(self, kind, x):
        net, dev = self.net, self.dev
        c, s, ns = net.in_nc, net.scale, self.ring.slots
        self.kind, self.in_cuda = kind, bool(x.is_cuda)
        if kind == 'yuv':
            self.h, self.w = self.yuv.h, self.yuv.w
        else:
            fmt = StreamFormat(kind, x)
            self.h, self.w = fmt.h, fmt.w
        h, w, m = self.h, self.w, max(self.first, self.later)
        self.wk = net._weights_key()
        self.plan = net._get_plan(1, h, w, dev, wk=self.wk)
        self.fplans = {}
        self.lib = L.lib()
        self.main = torch.cuda.current_stream(dev)
        self.side, self.copy = net._side_stream(dev), net._copy_stream(dev)
        self.lr = torch.empty(ns, m + 1, c, h, w, dtype=torch.float32, device=dev)      # [slot][0] = the frame before the batch
        self.hr = [torch.zeros(1, c, s * h, s * w, dtype=torch.float32, device=dev),
                   torch.empty(1, c, s * h, s * w, dtype=torch.float32, device=dev)]
        self.snap = torch.empty(ns, 1, c, s * h, s * w, dtype=torch.float32, device=dev)
        self.u8 = torch.empty(ns, m, s * h, s * w, c, dtype=torch.uint8, device=dev)
        ofb = self.yuv.out_frame_bytes(s) if kind == 'yuv' else s * h * s * w * c
        if self.png is not None:                    # per slot: m int64 sizes, then m regions of one file each
            cap, wsb = self.lib.tg_png_capacity(s * h, s * w), self.lib.tg_png_workspace_bytes(m, s * h, s * w)
            if cap < 0 or wsb < 0:
                L.check(L.TG_E_SHAPE, 'tg_png_capacity')
            self.png_stride = (cap + 7) // 8 * 8
            self.png_out = torch.empty(ns, 8 * m + m * self.png_stride, dtype=torch.uint8, device=dev)
            self.png_ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        self.host_out = torch.empty((ns, 8 * m + m * self.png_stride) if self.png is not None else
                                    (ns, m, ofb) if kind == 'yuv' else (ns, m, s * h, s * w, c), dtype=torch.uint8,
                                    pin_memory=True)
        if kind == 'yuv':                           # I420 both ways: 1.5 bytes per pixel through pinned memory
            self.stage = torch.empty(ns, m, self.yuv.frame_bytes, dtype=torch.uint8, pin_memory=True)
            self.dev_in = torch.empty(ns, m, self.yuv.frame_bytes, dtype=torch.uint8, device=dev)
            self.yuv_out = torch.empty(ns, m, ofb, dtype=torch.uint8, device=dev)
        elif kind == 'u8':
            self.stage = torch.empty(ns, m, h, w, c, dtype=torch.uint8, pin_memory=True)
            self.dev_in = torch.empty(ns, m, h, w, c, dtype=torch.uint8, device=dev)
        elif not self.in_cuda:
            self.stage = torch.empty(ns, m, c, h, w, dtype=torch.float32, pin_memory=True)
        self.zflow = torch.zeros(2 * self.plan.fh * self.plan.fw, dtype=torch.float32, device=dev)
        self.fsz = 2 * self.plan.fh * self.plan.fw * 4
        # what enqueue_batch is given: addresses per slot, and the bytes from one frame to the next
        self.lr_ptr, self.u8_ptr = [t.data_ptr() for t in self.lr], [t.data_ptr() for t in self.u8]
        self.lr_stride, self.u8_stride = c * h * w * 4, s * h * s * w * c
        self.hr_ptr = (self.hr[0].data_ptr(), self.hr[1].data_ptr())
        self.reset = None
        if self.scene_cut is not None:
            # per slot and frame: SAD (8 bytes), flag (4), histogram distance (4) -- one buffer, one download
            self.sc_out = torch.zeros(ns, 16 * m, dtype=torch.uint8, device=dev)
            self.sc_host = torch.zeros(ns, 16 * m, dtype=torch.uint8, pin_memory=True)
            self.sc_forced = torch.zeros(ns, m, dtype=torch.uint8, device=dev)
            self.sc_forced_host = torch.zeros(ns, m, dtype=torch.uint8, pin_memory=True)
            self.sc_wsb = self.lib.tg_scene_cut_workspace_bytes(m)
            self.sc_ws = torch.empty(ns, (self.sc_wsb + 7) // 8 * 8, dtype=torch.uint8, device=dev)
            self.sc_min = self.scene_cut.thresholds(h, w)
            self.reset = [(self.sc_out[sl].data_ptr() + 8 * m, self.hr[0].numel() * 4) for sl in range(ns)]
        ev = lambda: [torch.cuda.Event() for _ in range(ns)]
        self.ev_in, self.ev_f, self.ev_s, self.ev_out = ev(), ev(), ev(), ev()
        self.ev_arrive = torch.cuda.Event()
        self.side.wait_stream(self.main)            # weights, the zeroed state and the rings are ready
        self.copy.wait_stream(self.main)

    def _fplan(self, npair):
        fp = self.fplans.get(npair)
        if fp is None:
            if self.net._weights_key() != self.wk:
                raise RuntimeError('infer_stream: the weights changed while the stream was live')
            fp = self.fplans[npair] = self.net._get_plan(npair, self.h, self.w, self.dev, fnet_only=True, wk=self.wk)
        return fp

    # -- input ---------------------------------------------------------------------------------------------------
    def _take(self, b, off, piece):
        """A piece of the batch being filled: host frames into the slot's pinned staging (the caller's buffer is free
        again when this returns), device frames straight into the LR slot on the copy stream."""
        sl, n = self.ring.slot(b), piece.shape[0]
        if not self.in_cuda:
            self.stage[sl, off:off + n].copy_(piece)
            return
        piece = piece.contiguous()
        self.ev_arrive.record(torch.cuda.current_stream(self.dev))
        self.copy.wait_event(self.ev_arrive)
        with torch.cuda.stream(self.copy):
            self.lr[sl, 1 + off:1 + off + n].copy_(piece, non_blocking=True)
        piece.record_stream(self.copy)

    def _upload(self, rec):
        b, i0, cnt = rec
        sl = self.ring.slot(b)
        with torch.cuda.stream(self.copy):
            if b == 0:
                self.lr[sl, 0].zero_()                                   # frame -1 = zeros (reference tecogan_nets.py:266)
            else:
                pb, _, pcnt = self.prev_rec
                self.lr[sl, 0].copy_(self.lr[self.ring.slot(pb), pcnt], non_blocking=True)
            if self.kind == 'u8':
                self.dev_in[sl, :cnt].copy_(self.stage[sl, :cnt], non_blocking=True)
                L.check(self.lib.tg_dequantize_u8_hwc(self.dev_in[sl].data_ptr(), self.lr[sl, 1].data_ptr(), cnt,
                                                      self.net.in_nc, self.h, self.w, self.copy.cuda_stream),
                        'tg_dequantize_u8_hwc')
            elif self.kind == 'yuv':
                self.dev_in[sl, :cnt].copy_(self.stage[sl, :cnt], non_blocking=True)
                L.check(self.lib.tg_yuv420_to_rgb_f32(self.dev_in[sl].data_ptr(), self.lr[sl, 1].data_ptr(), cnt,
                                                      self.h, self.w, *self.yuv.codes(), self.copy.cuda_stream),
                        'tg_yuv420_to_rgb_f32')
            elif not self.in_cuda:
                self.lr[sl, 1:1 + cnt].copy_(self.stage[sl, :cnt], non_blocking=True)
            if self.scene_cut is not None:
                self._detect(sl, b, i0, cnt)
            self.ev_in[sl].record(self.copy)
        self.prev_rec = rec

    def _detect(self, sl, b, i0, cnt):
        """On the copy stream, behind the slot's LR frames: the forced mask goes up and tg_scene_cut_flags decides the
        batch's cnt pairs.  Frame 0 of the stream is never a cut: its pair (against the zero frame) is scored, its flag
        is cleared."""
        sc, m = self.scene_cut, self.sc_forced.shape[1]
        self.sc_forced_host[sl, :cnt].copy_(torch.from_numpy(sc.forced(i0, cnt)))
        self.sc_forced[sl, :cnt].copy_(self.sc_forced_host[sl, :cnt], non_blocking=True)
        out = self.sc_out[sl].data_ptr()
        L.check(self.lib.tg_scene_cut_flags(self.lr[sl].data_ptr(), cnt, self.h, self.w, self.sc_min[0], self.sc_min[1],
                                            self.sc_forced[sl].data_ptr(), 1 if sc.detect else 0, out + 8 * m, out,
                                            out + 12 * m, self.sc_ws[sl].data_ptr(), self.sc_wsb,
                                            self.copy.cuda_stream), 'tg_scene_cut_flags')
        if b == 0:
            self.sc_out[sl, 8 * m:8 * m + 4].zero_()

    # -- launches of one batch: infer_sequence(pipeline=True)'s, on this slot's buffers ---------------------------------
    def _compute(self, rec):
        b, i0, cnt = rec
        sl, ns = self.ring.slot(b), self.ring.slots
        main, side = self.main, self.side
        self._flush_download()                      # (of the batch before: its successor's upload is queued by now)
        side.wait_event(self.ev_in[sl])
        main.wait_event(self.ev_in[sl])
        with torch.cuda.stream(main):
            self.snap[sl].copy_(self.hr[i0 & 1], non_blocking=True)     # what a rerun of this batch starts from
        enqueue_batch(self.lib, self.plan, self._fplan, b, i0, cnt, self.lr_ptr[sl], self.lr_stride, self.hr_ptr,
                      self.u8_ptr[sl], self.u8_stride, self.zflow.data_ptr(), self.fsz, main, side, self.ev_f[sl],
                      self.ev_s[(b - 2) % ns] if b >= 2 else None,     # (flow slot b & 1 was batch b - 2's)
                      **({} if self.reset is None else {'reset': self.reset[sl]}))
        if self.yuv is not None:                    # the batch's RGB frames -> I420, behind its last frame
            s = self.net.scale
            L.check(self.lib.tg_rgb_u8_to_yuv420(self.u8[sl].data_ptr(), self.yuv_out[sl].data_ptr(), cnt,
                                                 s * self.h, s * self.w, *self.yuv.codes(), main.cuda_stream),
                    'tg_rgb_u8_to_yuv420')
        if self.png is not None:                    # the batch's RGB frames -> PNG files, behind its last frame
            s, base = self.net.scale, self.png_out[sl].data_ptr()
            L.check(self.lib.tg_png_encode_u8(self.u8[sl].data_ptr(), cnt, s * self.h, s * self.w, self.png.code(),
                                              base + 8 * self.u8.shape[1], self.png_stride, base,
                                              self.png_ws.data_ptr(), main.cuda_stream), 'tg_png_encode_u8')
        self.ev_s[sl].record(main)
        self.pending_dl = rec

    def _flush_download(self):
        """The download of the batch computed last goes onto the copy stream BEHIND the upload of the batch after it
        (when there is one): a download waits for its batch's last frame, and an upload queued behind it would hold the
        next flow pass back until then."""
        rec, self.pending_dl = self.pending_dl, None
        if rec is None:
            return
        b, _, cnt = rec
        sl = self.ring.slot(b)
        self.copy.wait_event(self.ev_s[sl])
        with torch.cuda.stream(self.copy):
            if self.png is not None:                # the sizes and the first cnt regions
                used = 8 * self.u8.shape[1] + cnt * self.png_stride
                self.host_out[sl, :used].copy_(self.png_out[sl, :used], non_blocking=True)
            else:
                done = self.yuv_out if self.yuv is not None else self.u8
                self.host_out[sl, :cnt].copy_(done[sl, :cnt], non_blocking=True)
            if self.scene_cut is not None:
                self.sc_host[sl].copy_(self.sc_out[sl], non_blocking=True)
            self.ev_out[sl].record(self.copy)

    # -- faults --------------------------------------------------------------------------------------------------
    @staticmethod
    def _timed_out(fn, *args):
        """Run fn; a recorded time-out of the one-launch body comes back as a value, every other error is raised."""
        try:
            fn(*args)
        except L.TecoganHipError as e:
            if 'timed out' not in str(e):
                raise
            return e
        return None

    def _drain(self):
        for st in (self.main, self.side, self.copy):
            st.synchronize()

    def _recover(self, err):
        """The frames enqueued since the last clean check are invalid: those of the batches in flight, never one that
        was yielded.  Drain, restore the HR state the oldest of them started from, and enqueue them all again with the
        plan's re-arm held off -- one launch per layer, which cannot time out."""
        if self.on_fault != 'rerun':
            raise err
        if not self.warned:
            import warnings
            warnings.warn('infer_stream: %s -- the batches in flight are computed again with one launch per layer' % err,
                          RuntimeWarning)
            self.warned = True
        self.reruns += 1
        self._drain()
        self.plan.chain_state()                     # faults of launches that were still queued: counted, not reported
        self.pending_dl = None                      # every batch in flight is downloaded again
        self.plan.hold_chain_rearm(True)
        try:
            _, i0, _ = self.ring.oldest()
            with torch.cuda.stream(self.main):
                self.hr[i0 & 1].copy_(self.snap[self.ring.slot(self.ring.oldest()[0])], non_blocking=True)
            for rec in list(self.ring.inflight):
                self._compute(rec)
        finally:
            self.plan.hold_chain_rearm(False)

    def _submit(self, cnt):
        rec = self.ring.submit(cnt)
        self._upload(rec)
        err = self._timed_out(self._compute, rec)
        if err is not None:
            self._recover(err)                      # (enqueues rec again as well: it is in flight)

    def _retire(self):
        b, _, cnt = self.ring.oldest()
        sl = self.ring.slot(b)
        while True:
            if self.pending_dl is not None and self.pending_dl[0] == b:
                self._flush_download()              # nothing came after it
            self.ev_out[sl].synchronize()
            err = self._timed_out(self.plan.check_chain)
            if err is None:
                break
            self._recover(err)
        _, i0, _ = self.ring.retire()
        if self.scene_cut is not None:
            m, res = self.sc_forced.shape[1], self.sc_host[sl].numpy()
            self.scene_cut.report(i0, res[8 * m:12 * m].view(np.int32)[:cnt], res[:8 * m].view(np.uint64)[:cnt],
                                  res[12 * m:].view(np.uint32)[:cnt], self.h * self.w)
        if self.png is not None:
            m, buf = self.u8.shape[1], self.host_out[sl].numpy()
            sizes = buf[:8 * m].view(np.int64)
            return [buf[8 * m + k * self.png_stride:8 * m + k * self.png_stride + int(sizes[k])] for k in range(cnt)]
        return self.host_out[sl, :cnt].numpy()

    # -- the generator -------------------------------------------------------------------------------------------
    def run(self):
        # (no torch.no_grad() around the yields: it would leak into the caller between them; nothing here records a graph)
        try:
            pending = 0                             # frames taken into the batch being filled
            for b, off, piece, full in stream_rebatch(stream_parts(self.frames, self.net.in_nc, self.yuv),
                                                      self.first, self.later):
                if self.plan is None:
                    self.net.check_faults()         # a fault of an EARLIER clip is never this stream's to repair
                    self._open('yuv' if self.yuv is not None else 'u8' if piece.dtype == torch.uint8 else 'f32', piece)
                self._take(b, off, piece)
                pending = off + piece.shape[0]
                if not full:
                    continue
                self._submit(pending)
                pending = 0
                if self.ring.full():
                    yield self._retire()
            if pending:
                self._submit(pending)               # the last batch: whatever is left
            while self.ring.inflight:
                yield self._retire()
        finally:
            self._close()

    def _close(self):
        self.closed = True
        if self.plan is None:
            return
        try:
            # the side and copy streams use memory the caching allocator knows only by its allocation stream:
            # nothing is released before all three are idle
            self._drain()
            self.main.wait_stream(self.side)
            self.main.wait_stream(self.copy)
            if self.ring.inflight:
                self.plan.chain_state()             # a fault in frames nobody will see: counted, the plan has fallen back
        finally:
            for name in ('lr', 'hr', 'snap', 'u8', 'host_out', 'stage', 'dev_in', 'yuv_out', 'png_out', 'png_ws', 'zflow',
                         'sc_out', 'sc_host', 'sc_forced', 'sc_forced_host', 'sc_ws'):
                self.__dict__.pop(name, None)
