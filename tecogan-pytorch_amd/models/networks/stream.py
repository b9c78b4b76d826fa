"""FRNet.infer_stream (DESIGN.md sections 7d, 7e, 7h, 7i, 7j, 7l, 7o): input parsing, the batch ring, the raw-video forms
Yuv420 and Yuv, the PNG output form Png, the scene-cut option SceneCut, the output size Resize, the interlaced-input
option Deinterlace with its batch-to-window mapping, one small object per input
form, output form and option, and the engine that runs a clip of any length through rings of STREAM_SLOTS batches.  A
batch's launches are frnet_infer's enqueue_batch, the ones infer_sequence(pipeline=True) enqueues.  Uses the network
only through its attributes."""
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from ... import _lib as L
from ...ops import YUV_SUBSAMPLING, yuv_frame_samples
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
    a chunk of frames.  With yuv.depth above 8 an item is the bytes of the file (uint8, frame_bytes a frame) or its
    samples (uint16, half that length), which are taken as their bytes.  Anything else is a ValueError."""
    x = item
    if yuv.depth > 8:
        if isinstance(x, np.ndarray) and x.dtype == np.uint16:
            x = np.ascontiguousarray(x).view(np.uint8)
        elif torch.is_tensor(x) and x.dtype == torch.uint16 and not x.is_cuda:
            x = x.contiguous().view(torch.uint8)
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


def stream_rebatch_sizes(parts, sizes):
    """stream_rebatch for batches that take sizes[0], sizes[1], ... input frames (an iterable that does not end).  A batch
    that takes none -- every frame it needs has arrived with the one before -- is handed out as (batch index, 0, None,
    True), directly behind the batch that completed it."""
    sizes = iter(sizes)
    b, fill, size = 0, 0, next(sizes)
    for _, x in parts:
        pos, n = 0, x.shape[0]
        while pos < n:
            m = min(size - fill, n - pos)
            piece, off = x[pos:pos + m], fill
            pos, fill = pos + m, fill + m
            full = fill == size
            yield b, off, piece, full
            if full:
                b, fill, size = b + 1, 0, next(sizes)
                while size == 0:
                    yield b, 0, None, True
                    b, size = b + 1, next(sizes)


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


YUV_DEPTHS = (8, 10, 12)
YUV_LAYOUTS = ('planar', 'semi')                 # U and V planes | one plane of interleaved U,V pairs


class _YuvSpec:
    """What Yuv420 and Yuv share: the validation of the fields (the messages carry the class's name), the derived sizes,
    and the C ABI's view of the spec.  A subclass names its matrices and its three launches -- input_launch(),
    out_launch(H, W) at 8 bits and deep_launch(H, W) above -- each as (entry point, the arguments between the frame
    count and the stream)."""

    def __post_init__(self):
        who = type(self).__name__
        for name in ('h', 'w'):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 2:
                raise ValueError(f'{who}: {name} is an integer >= 2, got {v!r}')
            object.__setattr__(self, name, int(v))
        for name, table in (('chroma', L.YUV_CHROMA), ('out_chroma', L.YUV_CHROMA), ('matrix', self.MATRICES),
                            ('siting', L.YUV_SITING)):
            v = getattr(self, name)
            if not (name == 'out_chroma' and v is None) and (not isinstance(v, str) or v not in table):
                raise ValueError(f'{who}: {name} is one of {sorted(table)}, got {v!r}')
        if not isinstance(self.full_range, (bool, np.bool_)):
            raise ValueError(f'{who}: full_range is a bool, got {self.full_range!r}')
        object.__setattr__(self, 'full_range', bool(self.full_range))
        for name in ('depth', 'out_depth'):
            v = getattr(self, name)
            if name == 'out_depth' and v is None:
                continue
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v not in YUV_DEPTHS:
                raise ValueError(f'{who}: {name} is one of {YUV_DEPTHS}, got {v!r}')
            object.__setattr__(self, name, int(v))
        for name in ('layout', 'out_layout'):
            v = getattr(self, name)
            if not (name == 'out_layout' and v is None) and (not isinstance(v, str) or v not in YUV_LAYOUTS):
                raise ValueError(f'{who}: {name} is one of {sorted(YUV_LAYOUTS)}, got {v!r}')

    @property
    def od(self):
        """Bits per sample of the output: out_depth, or the input's."""
        return self.depth if self.out_depth is None else self.out_depth

    @property
    def oc(self):
        """Layout of the output: out_chroma, or the input's."""
        return self.chroma if self.out_chroma is None else self.out_chroma

    @property
    def frame_bytes(self):
        return yuv_frame_samples(self.h, self.w, self.chroma) * (2 if self.depth > 8 else 1)

    def out_size_bytes(self, H, W):
        """Bytes of an H x W output frame; ValueError where the output layout cannot hold that size (4:2:0: even sides,
        4:2:2: an even width)."""
        sx, sy = YUV_SUBSAMPLING[self.oc]
        if H < 1 or W < 1 or H % sy or W % sx:
            raise ValueError(f'{type(self).__name__}: a 4:{self.oc[1]}:{self.oc[2]} output frame has '
                             f'{"even sides" if sy == 2 else "an even width"}, got {H}x{W}')
        return yuv_frame_samples(H, W, self.oc) * (2 if self.od > 8 else 1)

    def codes(self):
        """(matrix, full_range, siting) as the C ABI takes them."""
        return self.MATRICES[self.matrix], int(self.full_range), L.YUV_SITING[self.siting]


@dataclass(frozen=True)
class Yuv420(_YuvSpec):
    """Raw-video form of a stream (FRNet.infer_stream(yuv=...), DESIGN.md sections 7e and 7k): planar YUV 4:2:0 (I420)
    frames of h x w on the way in and of s*h x s*w on the way out.  matrix 'bt601' | 'bt709', full_range (bool),
    siting 'center' (y4m C420jpeg) | 'left' (y4m C420mpeg2).  depth 8 | 10 | 12: bits per sample of the input; above 8
    a sample is a 16-bit little-endian word.  out_depth 8 | 10 | 12 | None (the input's): bits per sample of the output;
    above 8 the frames are written from the float HR frame, not from the rounded uint8 one.  A Yuv420 takes the four
    4:2:0 entry points (tg_yuv420_to_rgb_f32, tg_yuv420p16_to_rgb_f32, tg_rgb_u8_to_yuv420, tg_rgb_f32_to_yuv420p16).
    Frozen."""
    h: int
    w: int
    matrix: str = 'bt709'
    full_range: bool = False
    siting: str = 'left'
    depth: int = 8
    out_depth: Optional[int] = None
    MATRICES, chroma, out_chroma = L.YUV_MATRIX, '420', None         # (no fields: the one layout, BT.601 / BT.709 only)
    layout, out_layout = 'planar', None

    def out_frame_bytes(self, scale):
        """Bytes of a super-resolved frame (s*h and s*w are even: the scale is 2 or 4)."""
        if scale < 1 or (scale * self.h) % 2 or (scale * self.w) % 2:
            raise ValueError(f'Yuv420: an output frame has even sides; scale {scale} gives {scale * self.h}x{scale * self.w}')
        return self.out_size_bytes(scale * self.h, scale * self.w)

    def input_launch(self):
        if self.depth > 8:
            return 'tg_yuv420p16_to_rgb_f32', (self.h, self.w, self.depth, *self.codes())
        return 'tg_yuv420_to_rgb_f32', (self.h, self.w, *self.codes())

    def out_launch(self, H, W):
        return 'tg_rgb_u8_to_yuv420', (H, W, *self.codes())

    def deep_launch(self, H, W):
        return 'tg_rgb_f32_to_yuv420p16', (H, W, self.od, *self.codes())


@dataclass(frozen=True)
class Yuv(_YuvSpec):
    """Raw-video form of a stream in any of the three planar layouts (FRNet.infer_stream(yuv=...), DESIGN.md section
    7l): frames of h x w on the way in and of s*h x s*w on the way out.  chroma '420' | '422' | '444': the layout of
    the input; out_chroma the same | None (the input's): the layout of the output.  matrix 'bt601' | 'bt709' | 'bt2020'
    (non-constant luminance), full_range (bool), siting 'center' | 'left': where a chroma sample sits along a
    sub-sampled horizontal axis (not looked at for 4:4:4).  depth and out_depth as Yuv420's.  Samples pass through as
    code values whatever their transfer function (PQ and HLG included).  A Yuv always takes the planar launches
    (tg_yuv_planar_to_rgb_f32, tg_rgb_u8_to_yuv_planar, tg_rgb_f32_to_yuv_planar16), at '420' as well.
    layout 'planar' | 'semi': the input's chroma as U and V planes, or as ONE plane of interleaved U,V pairs with the
    code in the top bits of a 16-bit word (NV12 / NV16 / NV24, P010 / P012, P210 / P212, P410 /
    P412); out_layout the same | None (the input's), independent of it.  A frame has the same bytes either way, and a
    semi-planar side takes the semi-planar launch in place of the planar one (tg_yuv_semiplanar_to_rgb_f32,
    tg_rgb_u8_to_yuv_semiplanar, tg_rgb_f32_to_yuv_semiplanar16).  Frozen."""
    h: int
    w: int
    chroma: str = '420'
    out_chroma: Optional[str] = None
    matrix: str = 'bt709'
    full_range: bool = False
    siting: str = 'left'
    depth: int = 8
    out_depth: Optional[int] = None
    layout: str = 'planar'
    out_layout: Optional[str] = None
    MATRICES = L.YUV_PLANAR_MATRIX

    @property
    def ol(self):
        """Chroma layout of the output: out_layout, or the input's."""
        return self.layout if self.out_layout is None else self.out_layout

    def out_frame_bytes(self, scale):
        """Bytes of a super-resolved frame."""
        if scale < 1:
            raise ValueError(f'Yuv: scale {scale}')
        return self.out_size_bytes(scale * self.h, scale * self.w)

    def input_launch(self):
        name = 'tg_yuv_semiplanar_to_rgb_f32' if self.layout == 'semi' else 'tg_yuv_planar_to_rgb_f32'
        return name, (self.h, self.w, L.YUV_CHROMA[self.chroma], self.depth, *self.codes())

    def out_launch(self, H, W):
        name = 'tg_rgb_u8_to_yuv_semiplanar' if self.ol == 'semi' else 'tg_rgb_u8_to_yuv_planar'
        return name, (H, W, L.YUV_CHROMA[self.oc], *self.codes())

    def deep_launch(self, H, W):
        name = 'tg_rgb_f32_to_yuv_semiplanar16' if self.ol == 'semi' else 'tg_rgb_f32_to_yuv_planar16'
        return name, (H, W, L.YUV_CHROMA[self.oc], self.od, *self.codes())


@dataclass(frozen=True)
class Png:
    """PNG output form of a stream (FRNet.infer_stream(png=...)): every super-resolved frame
    leaves the device as one complete 8-bit RGB PNG file, encoded there by tg_png_encode_u8.  filter 'adaptive' (per
    row the type with the smallest sum of |int8(byte)|) | 'none' (type 0 on every row).  Huffman-only deflate: the
    files are larger than zlib's.  lz77=True: tg_png_encode_lz_u8 instead, LZ77 matches inside
    every 32 KiB segment; no file is larger than without it, and the encoder takes longer.  Frozen."""
    filter: str = 'adaptive'
    lz77: bool = False

    def __post_init__(self):
        if not isinstance(self.filter, str) or self.filter not in L.PNG_FILTER:
            raise ValueError(f'Png: filter is one of {sorted(L.PNG_FILTER)}, got {self.filter!r}')
        if not isinstance(self.lz77, (bool, np.bool_)):
            raise ValueError(f'Png: lz77 is True or False, got {self.lz77!r}')
        object.__setattr__(self, 'lz77', bool(self.lz77))

    def entry(self):
        """(encoder, its workspace query) as the C ABI names them."""
        return ('tg_png_encode_lz_u8', 'tg_png_lz_workspace_bytes') if self.lz77 else \
            ('tg_png_encode_u8', 'tg_png_workspace_bytes')

    def code(self):
        """The filter as the C ABI takes it."""
        return L.PNG_FILTER[self.filter]


@dataclass(frozen=True)
class Resize:
    """Output size of a stream (FRNet.infer_stream(resize=...)): every super-resolved frame is
    resized to h x w on the device, by ONE tg_resample_u8 per batch (MATLAB-style antialiased bicubic, exact integers),
    before the output form sees it.  h / (s * LR height) and w / (s * LR width) lie in [1/4, 4].  Frozen."""
    h: int
    w: int

    def __post_init__(self):
        for name in ('h', 'w'):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
                raise ValueError(f'Resize: {name} is an integer >= 1, got {v!r}')
            object.__setattr__(self, name, int(v))

    def check_source(self, H, W):
        """ValueError unless H x W frames can be resized to h x w (either ratio in [1/4, 4])."""
        for n_in, n_out in ((H, self.h), (W, self.w)):
            if 4 * n_out < n_in or n_out > 4 * n_in:
                raise ValueError(f'resize: {H}x{W} frames to {self.h}x{self.w}: the ratio of either axis lies in [1/4, 4]')


DEINTERLACE_RATES = ('field', 'frame')


@dataclass(frozen=True)
class Deinterlace:
    """Interlaced input of a raw-video stream (FRNet.infer_stream(yuv=..., deinterlace=...)): the
    items are interlaced frames, and ONE tg_deinterlace_planar per batch, on the copy stream in front of the yuv
    launch, turns them into progressive frames -- an edge-directed line average bounded by a three-field motion measure,
    exact integers, the samples of tests/deinterlace_ref.py.  tff: the earlier field owns the even rows (top field
    first), else the odd ones.  rate 'field': two output frames per input frame, one per field, in time order;
    'frame': the input's rate, the earlier field's frame only.  **Not compared with ffmpeg's yadif or bwdif; the
    quarter-line vertical chroma offset of interlaced 4:2:0 is not modelled** (a deinterlaced frame is handed on as
    progressive).  Frozen."""
    tff: bool = True
    rate: str = 'field'

    def __post_init__(self):
        if not isinstance(self.tff, (bool, np.bool_)):
            raise ValueError(f'Deinterlace: tff is True or False, got {self.tff!r}')
        object.__setattr__(self, 'tff', bool(self.tff))
        if not isinstance(self.rate, str) or self.rate not in DEINTERLACE_RATES:
            raise ValueError(f'Deinterlace: rate is one of {sorted(DEINTERLACE_RATES)}, got {self.rate!r}')

    @property
    def per_frame(self):
        """Output frames per input frame."""
        return 2 if self.rate == 'field' else 1

    def check_source(self, yuv):
        """ValueError unless every plane of the spec's frames has both row parities: an even h, h % 4 == 0 at 4:2:0.
        Semi-planar input is refused: the edge directions step one sample sideways, which on interleaved chroma would
        mix U with V."""
        if getattr(yuv, 'layout', 'planar') != 'planar':
            raise ValueError("Deinterlace: interlaced semi-planar input (layout='semi') is not supported: the edge "
                             'directions of the deinterlacer step one sample sideways, which on interleaved chroma '
                             'would mix U with V; repack to planar')
        need = 4 if yuv.chroma == '420' else 2
        if yuv.h % need or yuv.h < 4:
            raise ValueError(f'Deinterlace: a 4:{yuv.chroma[1]}:{yuv.chroma[2]} frame needs a height that is a multiple of '
                             f'{need} and at least 4, got {yuv.h}')


def deinterlace_window(i0, cnt, rate='field'):
    """The input frames a batch of output frames i0 .. i0 + cnt - 1 of a deinterlaced stream is made from: (lo, hi,
    first_field).  lo is the frame BEFORE the first one that has a field in the batch (-1: there is none, the stream
    starts), hi the last one, first_field the field of frame lo + 1 the batch starts with.  At rate 'field' output i is
    field i % 2 of frame i // 2, so a frame's two fields may lie in two batches; at 'frame' output i is field 0 of frame
    i.  tg_deinterlace_planar takes frames lo .. hi as its k + 1 = hi - lo + 1 frames."""
    if rate == 'field':
        return i0 // 2 - 1, (i0 + cnt - 1) // 2, i0 & 1
    if rate == 'frame':
        return i0 - 1, i0 + cnt - 1, 0
    raise ValueError(f'deinterlace_window: rate is one of {sorted(DEINTERLACE_RATES)}, got {rate!r}')


def deinterlace_input_sizes(first, later, rate='field'):
    """Endlessly: the input frames that complete batch 0, 1, ... of a deinterlaced stream whose batches are `first`, then
    `later` output frames -- those up to the batch's hi that no batch before it took."""
    i0, cnt, have = 0, first, 0
    while True:
        need = deinterlace_window(i0, cnt, rate)[1] + 1 - have
        yield need
        i0, cnt, have = i0 + cnt, later, have + need


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


def yuv420_planes(chunk, H, W, depth=8):
    """yuv_planes of I420 frames: chunk (m, frame_bytes) -> (m,H,W), (m,ch,cw), (m,ch,cw); a single frame
    (frame_bytes,) -> (H,W), (ch,cw), (ch,cw)."""
    return yuv_planes(chunk, H, W, '420', depth, who='yuv420_planes')


def yuv_planes(chunk, H, W, chroma='420', depth=8, who='yuv_planes'):
    """(Y, U, V) views of planar frames in any of the three layouts, U and V of ceil(H/sy) x ceil(W/sx)
    with (sx, sy) = (2,2) '420', (2,1) '422', (1,1) '444'.  chunk (m, frame_bytes) or a single frame (frame_bytes,),
    numpy or torch; nothing is copied.  depth above 8: the chunk holds 2-byte samples (uint8 as the stream yields it, or
    uint16 already) and the views are uint16."""
    if chroma not in YUV_SUBSAMPLING:
        raise ValueError(f'{who}: chroma is one of {sorted(YUV_SUBSAMPLING)}, got {chroma!r}')
    if depth not in YUV_DEPTHS:
        raise ValueError(f'{who}: depth is one of {YUV_DEPTHS}, got {depth!r}')
    sx, sy = YUV_SUBSAMPLING[chroma]
    ch, cw = (H + sy - 1) // sy, (W + sx - 1) // sx
    ns = H * W + 2 * ch * cw
    if depth > 8 and chunk.dtype == (np.uint8 if isinstance(chunk, np.ndarray) else torch.uint8):
        if chunk.shape[-1] != 2 * ns:
            raise ValueError(f'{who}: {H}x{W} {chroma} frames at {depth} bits have {2 * ns} bytes; '
                             f'got shape {tuple(chunk.shape)}')
        chunk = chunk.view(np.uint16 if isinstance(chunk, np.ndarray) else torch.uint16)
    if chunk.shape[-1] != ns:
        raise ValueError(f'{who}: {H}x{W} {chroma} frames have {ns} samples; got shape {tuple(chunk.shape)}')
    lead = tuple(chunk.shape[:-1])
    return (chunk[..., :H * W].reshape(lead + (H, W)),
            chunk[..., H * W:H * W + ch * cw].reshape(lead + (ch, cw)),
            chunk[..., H * W + ch * cw:].reshape(lead + (ch, cw)))


def yuv_semiplanes(chunk, H, W, chroma='420', depth=8, who='yuv_semiplanes'):
    """(Y, UV) views of semi-planar frames: Y of H x W and UV of (ch, cw, 2) with ch x cw =
    ceil(H/sy) x ceil(W/sx), UV[..., 0] U and UV[..., 1] V.  chunk (m, frame_bytes) or a single frame (frame_bytes,),
    numpy or torch; nothing is copied.  depth above 8: the chunk holds 2-byte words (uint8 as the stream yields it, or
    uint16 already), the views are uint16 and the words are as stored, the code in the top bits (code << (16 - depth))."""
    y, u, v = yuv_planes(chunk, H, W, chroma, depth, who=who)       # (the checks, and the sizes: U and V have ch x cw each)
    ch, cw = u.shape[-2:]
    if chunk.shape[-1] != H * W + 2 * ch * cw:                      # bytes of 2-byte words, as the stream yields them
        chunk = chunk.view(np.uint16 if isinstance(chunk, np.ndarray) else torch.uint16)
    return y, chunk[..., H * W:].reshape(tuple(y.shape[:-2]) + (ch, cw, 2))


# -- the forms of a stream: each object owns its buffers and is the only place that knows their layout.  alloc(eng) runs
# once, inside the engine's _open; the engine decides when every other method runs, and on which stream (see there).
class _DeviceF32:
    """Input form: float32 frames on the device go straight into the LR slot on the copy stream; nothing is staged."""

    def __init__(self, h, w):
        self.h, self.w = h, w

    def alloc(self, eng):
        self.dev, self.copy, self.lr, self.ev_arrive = eng.dev, eng.copy, eng.lr, torch.cuda.Event()

    def take(self, sl, off, piece):
        piece = piece.contiguous()
        self.ev_arrive.record(torch.cuda.current_stream(self.dev))
        self.copy.wait_event(self.ev_arrive)
        with torch.cuda.stream(self.copy):
            self.lr[sl, 1 + off:1 + off + piece.shape[0]].copy_(piece, non_blocking=True)
        piece.record_stream(self.copy)

    def upload(self, sl, i0, cnt):
        pass


class _HostF32:
    """Input form: float32 frames on the host, through pinned staging (the caller's buffer is free again when take
    returns) into the LR slot."""

    def __init__(self, h, w):
        self.h, self.w = h, w

    def alloc(self, eng):
        self.lr = eng.lr
        self.stage = torch.empty(eng.ring.slots, eng.m, eng.net.in_nc, self.h, self.w, dtype=torch.float32, pin_memory=True)

    def take(self, sl, off, piece):
        self.stage[sl, off:off + piece.shape[0]].copy_(piece)

    def upload(self, sl, i0, cnt):
        self.lr[sl, 1:1 + cnt].copy_(self.stage[sl, :cnt], non_blocking=True)


class _HostBytes:
    """Input form: uint8 frames on the host go up as bytes, through pinned staging, and ONE launch converts a batch
    into the LR slot: `launch`(bytes, LR frames, cnt, *args, stream).  uint8 RGB frames and I420 frames differ only in
    that launch and in the shape of a frame."""

    def __init__(self, h, w, frame_shape, launch, args):
        self.h, self.w, self.frame_shape, self.launch, self.args = h, w, frame_shape, launch, args

    def alloc(self, eng):
        self.lr, self.fn, self.stream = eng.lr, getattr(eng.lib, self.launch), eng.copy.cuda_stream
        self.stage = torch.empty(eng.ring.slots, eng.m, *self.frame_shape, dtype=torch.uint8, pin_memory=True)
        self.dev_in = torch.empty(eng.ring.slots, eng.m, *self.frame_shape, dtype=torch.uint8, device=eng.dev)

    def take(self, sl, off, piece):
        self.stage[sl, off:off + piece.shape[0]].copy_(piece)

    def upload(self, sl, i0, cnt):
        self.dev_in[sl, :cnt].copy_(self.stage[sl, :cnt], non_blocking=True)
        L.check(self.fn(self.dev_in[sl].data_ptr(), self.lr[sl, 1].data_ptr(), cnt, *self.args, self.stream), self.launch)


class _InterlacedBytes:
    """Input form: interlaced planar YUV frames on the host.  A batch of cnt OUTPUT frames takes
    the input frames deinterlace_window names; the ones no earlier batch took go up as bytes through pinned staging into
    entries 2.. of the slot's raw frames, and entries 0 and 1 are the two frames before them, copied on the device from
    the slot of the batch before (entry e of a slot is input frame `first new frame - 2 + e`: the layout is defined here
    and nowhere else).  Then ONE tg_deinterlace_planar writes the slot's cnt progressive frames and the spec's own
    input launch converts those into the LR slot, all on the copy stream."""

    def __init__(self, yuv, deint):
        self.h, self.w, self.yuv, self.deint = yuv.h, yuv.w, yuv, deint
        self.launch, self.args = yuv.input_launch()

    def alloc(self, eng):
        ns, m, fb = eng.ring.slots, eng.m, self.yuv.frame_bytes
        self.lr, self.fn, self.stream = eng.lr, getattr(eng.lib, self.launch), eng.copy.cuda_stream
        self.fn_deint = eng.lib.tg_deinterlace_planar
        self.deint_args = (self.h, self.w, L.YUV_CHROMA[self.yuv.chroma], self.yuv.depth, 1 if self.deint.tff else 0)
        self.stage = torch.empty(ns, m, fb, dtype=torch.uint8, pin_memory=True)
        self.raw = torch.empty(ns, m + 2, fb, dtype=torch.uint8, device=eng.dev)
        self.prog = torch.empty(ns, m, fb, dtype=torch.uint8, device=eng.dev)
        self.fb, self.taken, self.prev_slot = fb, 0, None       # taken: input frames uploaded so far

    def take(self, sl, off, piece):
        self.stage[sl, off:off + piece.shape[0]].copy_(piece)

    def upload(self, sl, i0, cnt):
        lo, hi, first_field = deinterlace_window(i0, cnt, self.deint.rate)
        new, at = hi + 1 - self.taken, lo - (self.taken - 2)    # at: the slot's entry of frame lo
        if new < 0 or new > self.stage.shape[1] or at not in (0, 1):
            raise RuntimeError(f'infer_stream: batch {i0}+{cnt} needs frames {lo}..{hi} with {self.taken} taken')
        if self.prev_slot is not None:
            psl, pnew = self.prev_slot
            self.raw[sl, :2].copy_(self.raw[psl, pnew:pnew + 2], non_blocking=True)
        if new:
            self.raw[sl, 2:2 + new].copy_(self.stage[sl, :new], non_blocking=True)
        step = 1 if self.deint.rate == 'field' else 2
        L.check(self.fn_deint(self.raw[sl, at].data_ptr(), self.prog[sl].data_ptr(), hi - lo, *self.deint_args,
                              1 if lo >= 0 else 0, first_field, step, cnt, self.stream), 'tg_deinterlace_planar')
        L.check(self.fn(self.prog[sl].data_ptr(), self.lr[sl, 1].data_ptr(), cnt, *self.args, self.stream), self.launch)
        self.taken, self.prev_slot = hi + 1, (sl, new)


def _input_form(piece, c, yuv, deint=None):
    """The input form of a stream, from its options and its first item (as stream_parts hands it out)."""
    if deint is not None:
        return _InterlacedBytes(yuv, deint)
    if yuv is not None:
        return _HostBytes(yuv.h, yuv.w, (yuv.frame_bytes,), *yuv.input_launch())
    if piece.dtype == torch.uint8:
        h, w = piece.shape[1:3]
        return _HostBytes(h, w, (h, w, c), 'tg_dequantize_u8_hwc', (c, h, w))
    return (_DeviceF32 if piece.is_cuda else _HostF32)(piece.shape[2], piece.shape[3])


class _RgbOut:
    """Output form: the batch's uint8 RGB frames come down as they are; the chunk is a view of the pinned slot."""

    def alloc(self, eng):
        self.u8 = eng.out_u8
        self.host_out = torch.empty(tuple(self.u8.shape), dtype=torch.uint8, pin_memory=True)

    def encode(self, sl, cnt):
        pass

    def download(self, sl, cnt):
        self.host_out[sl, :cnt].copy_(self.u8[sl, :cnt], non_blocking=True)

    def result(self, sl, cnt):
        return self.host_out[sl, :cnt].numpy()


class _YuvOut:
    """Output form planar YUV at 8 bits (DESIGN.md sections 7e and 7l): ONE launch of the spec's out_launch
    (tg_rgb_u8_to_yuv420 for a Yuv420, tg_rgb_u8_to_yuv_planar for a Yuv) turns the batch's RGB frames into the slot's
    YUV frames on the device, and those come down: out_size_bytes per frame, on the device and pinned."""

    def __init__(self, yuv):
        self.yuv = yuv

    def alloc(self, eng):
        ns, m, H, W = eng.out_u8.shape[:4]
        self.u8, (self.launch, args) = eng.out_u8, self.yuv.out_launch(H, W)
        self.fn, self.args = getattr(eng.lib, self.launch), (*args, eng.main.cuda_stream)
        self.host_out = torch.empty(ns, m, self.yuv.out_size_bytes(H, W), dtype=torch.uint8, pin_memory=True)
        self.yuv_out = torch.empty(tuple(self.host_out.shape), dtype=torch.uint8, device=eng.dev)

    def encode(self, sl, cnt):
        L.check(self.fn(self.u8[sl].data_ptr(), self.yuv_out[sl].data_ptr(), cnt, *self.args), self.launch)

    def download(self, sl, cnt):
        self.host_out[sl, :cnt].copy_(self.yuv_out[sl, :cnt], non_blocking=True)

    def result(self, sl, cnt):
        return self.host_out[sl, :cnt].numpy()


class _YuvDeepOut:
    """Output form planar YUV at 10 or 12 bits (DESIGN.md sections 7k and 7l): directly behind every frame's SRNet
    launch ONE launch of the spec's deep_launch (tg_rgb_f32_to_yuv420p16 for a Yuv420, tg_rgb_f32_to_yuv_planar16 for a
    Yuv; n = 1, on the caller's stream) converts the float HR frame just written into the slot's device buffer at that
    frame -- `after(sl)` is the hook enqueue_batch calls -- so nothing is left to encode behind the batch.  The slot's
    uint8 frames are still written by the HR tail and are not downloaded."""

    def __init__(self, yuv):
        self.yuv = yuv

    def alloc(self, eng):
        ns, m, H, W = eng.u8.shape[:4]
        self.fb = self.yuv.out_frame_bytes(eng.net.scale)
        self.launch, args = self.yuv.deep_launch(H, W)
        self.fn, self.args = getattr(eng.lib, self.launch), (1, *args, eng.main.cuda_stream)
        self.host_out = torch.empty(ns, m, self.fb, dtype=torch.uint8, pin_memory=True)
        self.yuv_out = torch.empty(ns, m, self.fb, dtype=torch.uint8, device=eng.dev)

    def after(self, sl):
        base, fb, fn, args, launch = self.yuv_out[sl].data_ptr(), self.fb, self.fn, self.args, self.launch

        def convert(j, hr_addr):
            L.check(fn(hr_addr, base + j * fb, *args), launch)
        return convert

    def encode(self, sl, cnt):
        pass

    def download(self, sl, cnt):
        self.host_out[sl, :cnt].copy_(self.yuv_out[sl, :cnt], non_blocking=True)

    def result(self, sl, cnt):
        return self.host_out[sl, :cnt].numpy()


class _PngOut:
    """Output form PNG.  A slot, on the device and pinned, is m int64 file sizes followed by m
    regions of png_stride bytes (tg_png_capacity rounded up to 8), file k from the first byte of region k: the layout is
    defined here and nowhere else.  ONE tg_png_encode_u8 (tg_png_encode_lz_u8 for Png(lz77=True), section 7n, with its own
    workspace size) writes a batch's files and sizes; the sizes and the first cnt
    regions come down; the chunk is a list of views cut from the pinned slot by the sizes.  The encoder's workspace is
    one for all slots: every call is on the caller's stream."""

    def __init__(self, png):
        self.png = png

    def layout(self, m, cap):
        self.m, self.png_stride = m, (cap + 7) // 8 * 8
        self.files_at, self.slot_bytes = 8 * m, 8 * m + m * self.png_stride

    def alloc(self, eng):
        ns, m, H, W = eng.out_u8.shape[:4]
        self.fn_name, ws_name = self.png.entry()
        self.fn = getattr(eng.lib, self.fn_name)
        cap, wsb = eng.lib.tg_png_capacity(H, W), getattr(eng.lib, ws_name)(m, H, W)
        if cap < 0 or wsb < 0:
            L.check(L.TG_E_SHAPE, 'tg_png_capacity')
        self.layout(m, cap)
        self.lib, self.u8, self.size, self.stream = eng.lib, eng.out_u8, (H, W), eng.main.cuda_stream
        self.png_out = torch.empty(ns, self.slot_bytes, dtype=torch.uint8, device=eng.dev)
        self.png_ws = torch.empty(wsb, dtype=torch.uint8, device=eng.dev)
        self.host_out = torch.empty(ns, self.slot_bytes, dtype=torch.uint8, pin_memory=True)

    def encode(self, sl, cnt):
        base = self.png_out[sl].data_ptr()
        L.check(self.fn(self.u8[sl].data_ptr(), cnt, *self.size, self.png.code(), base + self.files_at, self.png_stride,
                        base, self.png_ws.data_ptr(), self.stream), self.fn_name)

    def download(self, sl, cnt):
        used = self.files_at + cnt * self.png_stride
        self.host_out[sl, :used].copy_(self.png_out[sl, :used], non_blocking=True)

    def result(self, sl, cnt):
        buf = self.host_out[sl].numpy()
        sizes = buf[:self.files_at].view(np.int64)
        at = [self.files_at + k * self.png_stride for k in range(cnt)]
        return [buf[a:a + int(sizes[k])] for k, a in enumerate(at)]


class _CutSlots:
    """The scene-cut slots of a stream with a SceneCut.  A slot's result record, on the device
    and pinned, is m uint64 SADs at byte 0, m int32 flags at 8 m and m uint32 histogram distances at 12 m -- one buffer,
    one download; the layout is defined here and nowhere else.  A slot also has the forced mask (device and pinned) and
    the detector's workspace."""

    def __init__(self, scene_cut):
        self.sc = scene_cut

    def layout(self, m):
        self.m, self.flags_at, self.dist_at, self.slot_bytes = m, 8 * m, 12 * m, 16 * m

    def alloc(self, eng):
        ns, m, dev = eng.ring.slots, eng.m, eng.dev
        self.layout(m)
        self.lib, self.lr, self.stream, self.h, self.w = eng.lib, eng.lr, eng.copy.cuda_stream, eng.h, eng.w
        self.n_pixels, self.hr_bytes = eng.h * eng.w, eng.hr[0].numel() * 4
        self.sc_out = torch.zeros(ns, self.slot_bytes, dtype=torch.uint8, device=dev)
        self.sc_host = torch.zeros(ns, self.slot_bytes, dtype=torch.uint8, pin_memory=True)
        self.sc_forced = torch.zeros(ns, m, dtype=torch.uint8, device=dev)
        self.sc_forced_host = torch.zeros(ns, m, dtype=torch.uint8, pin_memory=True)
        self.sc_wsb = self.lib.tg_scene_cut_workspace_bytes(m)
        self.sc_ws = torch.empty(ns, (self.sc_wsb + 7) // 8 * 8, dtype=torch.uint8, device=dev)
        self.sc_min = self.sc.thresholds(eng.h, eng.w)

    def detect(self, sl, b, i0, cnt):
        """Behind the slot's LR frames: the forced mask goes up and tg_scene_cut_flags decides the batch's cnt pairs.
        Frame 0 of the stream is never a cut: its pair (against the zero frame) is scored, its flag is cleared."""
        self.sc_forced_host[sl, :cnt].copy_(torch.from_numpy(self.sc.forced(i0, cnt)))
        self.sc_forced[sl, :cnt].copy_(self.sc_forced_host[sl, :cnt], non_blocking=True)
        out = self.sc_out[sl].data_ptr()
        L.check(self.lib.tg_scene_cut_flags(self.lr[sl].data_ptr(), cnt, self.h, self.w, self.sc_min[0], self.sc_min[1],
                                            self.sc_forced[sl].data_ptr(), 1 if self.sc.detect else 0, out + self.flags_at,
                                            out, out + self.dist_at, self.sc_ws[sl].data_ptr(), self.sc_wsb, self.stream),
                'tg_scene_cut_flags')
        if b == 0:
            self.sc_out[sl, self.flags_at:self.flags_at + 4].zero_()

    def reset(self, sl):
        """(address of the slot's flags, bytes of the HR state): what enqueue_batch takes as `reset`."""
        return self.sc_out[sl].data_ptr() + self.flags_at, self.hr_bytes

    def download(self, sl):
        self.sc_host[sl].copy_(self.sc_out[sl], non_blocking=True)

    def report(self, sl, i0, cnt):
        res = self.sc_host[sl].numpy()
        self.sc.report(i0, res[self.flags_at:self.dist_at].view(np.int32)[:cnt], res[:self.flags_at].view(np.uint64)[:cnt],
                       res[self.dist_at:].view(np.uint32)[:cnt], self.n_pixels)


class _ResizedFrames:
    """The resized frames of a stream with a Resize: one more uint8 ring, (slots, m, h, w, 3), and
    the two axes' tables on the device.  ONE tg_resample_u8 per batch turns the slot's HR frames into the slot's resized
    frames; the output form reads those (eng.out_u8) in place of the HR frames."""

    def __init__(self, resize):
        self.rs = resize

    def alloc(self, eng):
        from ... import ops
        ns, m, H, W = eng.u8.shape[:4]
        self.lib, self.u8 = eng.lib, eng.u8
        vi, vw, vt = ops.resample_tables_device(H, self.rs.h, eng.dev)
        hi, hw, ht = ops.resample_tables_device(W, self.rs.w, eng.dev)
        self.tables = (vi, vw, hi, hw)              # (kept alive: the cache may drop them)
        self.args = (H, W, self.rs.h, self.rs.w, vi.data_ptr(), vw.data_ptr(), vt, hi.data_ptr(), hw.data_ptr(), ht,
                     eng.main.cuda_stream)
        self.frames = torch.empty(ns, m, self.rs.h, self.rs.w, 3, dtype=torch.uint8, device=eng.dev)

    def run(self, sl, cnt):
        L.check(self.lib.tg_resample_u8(self.u8[sl].data_ptr(), self.frames[sl].data_ptr(), cnt, *self.args),
                'tg_resample_u8')


class _StreamEngine:
    """State of one FRNet.infer_stream (see there): the part that is the same for every form.  Everything the device
    touches is allocated once, at the first item: STREAM_SLOTS slots of {LR batch + the frame before it, uint8 frames on
    the device, HR state snapshot, four events}, the HR ping-pong pair, the zero flow, and what the three form objects
    above allocate for themselves -- `inp` (staging and raw input), `out` (the pinned output ring and what is encoded
    into it), `cut` (None without a SceneCut), `rsz` (the resized ring, None without a Resize).  Per batch:

    _upload, copy stream: the frame before the batch, inp.upload, cut.detect, ev_in.
    _compute, caller's stream: the HR snapshot, enqueue_batch (given cut.reset: one tg_zero_if_flag in front of every
    frame's SRNet launch; given deep.after, 10- and 12-bit output only: one conversion behind it), rsz.run and then
    out.encode behind the batch's last frame, ev_s.
    _flush_download, copy stream, behind the NEXT batch's upload or at retire: out.download, cut.download, ev_out.
    _retire: waits for ev_out, reads the fault counter, cut.report, returns out.result.

    The host never waits for a scene-cut decision.  The repair path knows no form: it runs _compute again, which
    resizes and encodes again and reads the same per-slot flags, and the snapshot it restores was taken before the
    batch's first conditional fill."""

    def __init__(self, net, frames, device, on_fault, yuv=None, scene_cut=None, png=None, resize=None, deinterlace=None):
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
            if not isinstance(yuv, (Yuv420, Yuv)):
                raise ValueError(f'yuv must be a Yuv420, a Yuv or None, got {type(yuv).__name__}')
            yuv.out_frame_bytes(net.scale)
        if deinterlace is not None:
            if not isinstance(deinterlace, Deinterlace):
                raise ValueError(f'deinterlace must be a Deinterlace or None, got {type(deinterlace).__name__}')
            if yuv is None:
                raise ValueError('infer_stream: deinterlace works on planar YUV frames; pass yuv (a Yuv420 or a Yuv) with it')
            deinterlace.check_source(yuv)
        if scene_cut is not None:
            if not isinstance(scene_cut, SceneCut):
                raise ValueError(f'scene_cut must be a SceneCut or None, got {type(scene_cut).__name__}')
            if net.in_nc != 3:
                raise ValueError(f'scene_cut needs RGB frames (in_nc = 3), this network has in_nc = {net.in_nc}')
            scene_cut.cuts.clear()
            scene_cut.scores.clear()
        if resize is not None:
            if not isinstance(resize, Resize):
                raise ValueError(f'resize must be a Resize or None, got {type(resize).__name__}')
            if net.in_nc != 3:
                raise ValueError(f'resize needs RGB frames (in_nc = 3), this network has in_nc = {net.in_nc}')
            if isinstance(yuv, Yuv):
                if yuv.od == 8:
                    yuv.out_size_bytes(resize.h, resize.w)          # (per layout: 4:2:2 an even width, 4:4:4 any size)
            elif yuv is not None:
                if resize.h % 2 or resize.w % 2:
                    raise ValueError(f'resize: an I420 frame has even sides, got {resize.h}x{resize.w}')
            if yuv is not None:
                if yuv.od > 8:
                    raise ValueError(f'infer_stream: resize works on the 8-bit frames and cannot be combined with '
                                     f'out_depth = {yuv.od}; resize needs an 8-bit output')
                resize.check_source(net.scale * yuv.h, net.scale * yuv.w)
        # the forms: the output and the scene-cut slots follow from the options, the input from the first item as well
        self.inp, self.input_form = None, lambda piece: _input_form(piece, net.in_nc, yuv, deinterlace)
        self.deint, self.n_in = deinterlace, 0
        self.deep = None if yuv is None or yuv.od == 8 else _YuvDeepOut(yuv)        # (per-frame hook)
        self.out = _PngOut(png) if png is not None else self.deep if self.deep is not None else \
            _YuvOut(yuv) if yuv is not None else _RgbOut()
        self.cut = _CutSlots(scene_cut) if scene_cut is not None else None
        self.rsz = _ResizedFrames(resize) if resize is not None else None
        self.net, self.on_fault, self.parts = net, on_fault, stream_parts(frames, net.in_nc, yuv)
        self.dev = _norm_device(device if device is not None else next(net.parameters()).device)
        self.closed, self.warned, self.reruns = False, False, 0
        self.ring = StreamRing()
        self.first, self.later = stream_batch_sizes()
        self.plan, self.pending_dl, self.prev_rec = None, None, None

    # -- allocation (once) ---------------------------------------------------------------------------------------
    def _open(self, piece):
        net, dev = self.net, self.dev
        self.inp = self.input_form(piece)
        c, s, ns = net.in_nc, net.scale, self.ring.slots
        h, w, m = self.inp.h, self.inp.w, max(self.first, self.later)
        self.h, self.w, self.m = h, w, m
        if self.rsz is not None:
            self.rsz.rs.check_source(s * h, s * w)  # (the size of the first item: nothing has been allocated or enqueued)
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
        self.out_u8 = self.u8                       # what the output form reads
        if self.rsz is not None:
            self.rsz.alloc(self)
            self.out_u8 = self.rsz.frames
        self.out.alloc(self)
        self.inp.alloc(self)
        self.zflow = torch.zeros(2 * self.plan.fh * self.plan.fw, dtype=torch.float32, device=dev)
        self.fsz = 2 * self.plan.fh * self.plan.fw * 4
        # what enqueue_batch is given: addresses per slot, and the bytes from one frame to the next
        self.lr_ptr, self.u8_ptr = [t.data_ptr() for t in self.lr], [t.data_ptr() for t in self.u8]
        self.lr_stride, self.u8_stride = c * h * w * 4, s * h * s * w * c
        self.hr_ptr = (self.hr[0].data_ptr(), self.hr[1].data_ptr())
        if self.cut is not None:
            self.cut.alloc(self)
        ev = lambda: [torch.cuda.Event() for _ in range(ns)]
        self.ev_in, self.ev_f, self.ev_s, self.ev_out = ev(), ev(), ev(), ev()
        self.side.wait_stream(self.main)            # weights, the zeroed state and the rings are ready
        self.copy.wait_stream(self.main)

    def _fplan(self, npair):
        fp = self.fplans.get(npair)
        if fp is None:
            if self.net._weights_key() != self.wk:
                raise RuntimeError('infer_stream: the weights changed while the stream was live')
            fp = self.fplans[npair] = self.net._get_plan(npair, self.h, self.w, self.dev, fnet_only=True, wk=self.wk)
        return fp

    # -- launches of one batch: infer_sequence(pipeline=True)'s, on this slot's buffers ---------------------------------
    def _upload(self, rec):
        b, i0, cnt = rec
        sl = self.ring.slot(b)
        with torch.cuda.stream(self.copy):
            if b == 0:
                self.lr[sl, 0].zero_()                                   # frame -1 = zeros (reference tecogan_nets.py:266)
            else:
                pb, _, pcnt = self.prev_rec
                self.lr[sl, 0].copy_(self.lr[self.ring.slot(pb), pcnt], non_blocking=True)
            self.inp.upload(sl, i0, cnt)
            if self.cut is not None:
                self.cut.detect(sl, b, i0, cnt)     # behind whatever wrote the slot's LR frames
            self.ev_in[sl].record(self.copy)
        self.prev_rec = rec

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
                      reset=self.cut.reset(sl) if self.cut is not None else None,
                      after=self.deep.after(sl) if self.deep is not None else None)
        if self.rsz is not None:
            self.rsz.run(sl, cnt)                   # behind the batch's last frame, in front of the encode
        self.out.encode(sl, cnt)                    # behind the batch's last frame
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
            self.out.download(sl, cnt)
            if self.cut is not None:
                self.cut.download(sl)
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
        if self.cut is not None:
            self.cut.report(sl, i0, cnt)
        return self.out.result(sl, cnt)

    # -- the generator -------------------------------------------------------------------------------------------
    def _rebatch(self):
        """The input cut into batches: a batch's own frames, or with a Deinterlace the input frames its window adds."""
        if self.deint is None:
            return stream_rebatch(self.parts, self.first, self.later)
        return stream_rebatch_sizes(self.parts, deinterlace_input_sizes(self.first, self.later, self.deint.rate))

    def _batch_frames(self, pending, full):
        """Output frames of the batch that holds `pending` input frames: as many -- or with a Deinterlace a full batch's
        size, and at the end of the input every output frame that is still owed."""
        if self.deint is None:
            return pending
        if full:
            return self.later if self.ring.next_batch else self.first
        return self.n_in * self.deint.per_frame - self.ring.next_frame

    def run(self):
        # (no torch.no_grad() around the yields: it would leak into the caller between them; nothing here records a graph)
        try:
            pending = 0                             # frames taken into the batch being filled
            for b, off, piece, full in self._rebatch():
                if self.plan is None:
                    self.net.check_faults()         # a fault of an EARLIER clip is never this stream's to repair
                    self._open(piece)
                if piece is not None:               # (None: a deinterlaced batch whose frames all arrived before)
                    self.inp.take(self.ring.slot(b), off, piece)
                    pending = off + piece.shape[0]
                    self.n_in += piece.shape[0]
                if not full:
                    continue
                self._submit(self._batch_frames(pending, True))
                pending = 0
                if self.ring.full():
                    yield self._retire()
            tail = self._batch_frames(pending, False)
            if tail:
                self._submit(tail)                  # the last batch: whatever is left
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
            self.inp = self.out = self.deep = self.cut = self.rsz = None   # the forms' buffers go with them
            self.lr = self.hr = self.snap = self.u8 = self.out_u8 = self.zflow = None

