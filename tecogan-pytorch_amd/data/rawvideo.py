"""Headerless raw video in the semi-planar formats hardware decoders and encoders exchange: what
`ffmpeg -f rawvideo -pix_fmt nv12` writes and reads -- frame after frame, nothing in between, so the format and the
size come from the command line.  y4m cannot carry these layouts.

A frame of h x w is the Y plane, then ONE plane of ceil(h/sy) rows of 2 * ceil(w/sx) samples, U and V interleaved; a
sample is a byte at 8 bits and above a 16-bit little-endian word with the code in its top bits."""
import numpy as np

# ffmpeg's pixel-format names -> (chroma, depth); the p-formats are the little-endian ones (p010le, ...), whose names
# are taken with or without the suffix
FORMATS = {'nv12': ('420', 8), 'nv16': ('422', 8), 'nv24': ('444', 8),
           'p010': ('420', 10), 'p012': ('420', 12), 'p210': ('422', 10), 'p212': ('422', 12),
           'p410': ('444', 10), 'p412': ('444', 12)}
FORMAT_OF = {v: k for k, v in FORMATS.items()}
SUBSAMPLING = {'420': (2, 2), '422': (2, 1), '444': (1, 1)}         # chroma -> (sx, sy)


class RawVideoError(ValueError):
    pass


def format_of(name):
    """A format name (`nv12`, `p010`, `p010le`, any case) -> (chroma, depth); RawVideoError for anything else."""
    key = name.lower() if isinstance(name, str) else name
    if isinstance(key, str) and key.endswith('le') and key[:-2] in FORMATS and key[0] == 'p':
        key = key[:-2]
    if key not in FORMATS:
        raise RawVideoError(f'rawvideo: format is one of {" ".join(FORMATS)}, got {name!r}')
    return FORMATS[key]


def frame_bytes(h, w, chroma='420', depth=8):
    sx, sy = SUBSAMPLING[chroma]
    return (h * w + 2 * ((h + sy - 1) // sy) * ((w + sx - 1) // sx)) * (2 if depth > 8 else 1)


class RawReader:
    """Frames of a headerless stream of `fmt` frames of w x h, lazily: iterating yields ONE reused (frame_bytes,) uint8
    numpy buffer per frame (copy what you keep; FRNet.infer_stream copies an item when it pulls it).  fileobj: anything
    with read / readinto.  Short reads are looped over; the end of the stream at a frame boundary ends the iteration,
    inside a frame it is an error that names the byte count."""

    def __init__(self, fileobj, fmt, w, h):
        self.f = fileobj
        self.chroma, self.depth = format_of(fmt)
        if isinstance(w, bool) or isinstance(h, bool) or not isinstance(w, int) or not isinstance(h, int) or w < 2 or h < 2:
            raise RawVideoError(f'rawvideo: the size is W x H, two integers of at least 2 (got W={w!r} H={h!r})')
        self.w, self.h = w, h
        self.frame_bytes = frame_bytes(h, w, self.chroma, self.depth)
        self.frames_read = 0
        self._buf = np.empty(self.frame_bytes, np.uint8)

    def __iter__(self):
        return self

    def __next__(self):
        view, got, n = memoryview(self._buf), 0, self.frame_bytes
        readinto = getattr(self.f, 'readinto', None)
        while got < n:
            if readinto is not None:
                k = readinto(view[got:])
            else:
                piece = self.f.read(n - got)
                k = len(piece)
                view[got:got + k] = piece
            if not k:
                if got == 0:
                    raise StopIteration
                raise RawVideoError(f'rawvideo: the stream ends inside frame {self.frames_read}: {got} of {n} bytes')
            got += k
        self.frames_read += 1
        return self._buf


class RawWriter:
    """Writes frames one behind the other, nothing in between: any contiguous buffer per frame (uint8, or uint16 words
    above 8 bits).  frame_bytes, if given, is what every frame must have."""

    def __init__(self, fileobj, frame_bytes=None):
        self.f, self.frame_bytes, self.frames_written = fileobj, frame_bytes, 0

    def write(self, frame):
        view = memoryview(np.ascontiguousarray(frame)).cast('B')
        if self.frame_bytes is not None and len(view) != self.frame_bytes:
            raise RawVideoError(f'rawvideo: a frame has {self.frame_bytes} bytes, got {len(view)}')
        while len(view):                            # (an unbuffered pipe may take less than it is given)
            k = self.f.write(view)
            view = view[len(view) if k is None else k:]
        self.frames_written += 1

    def flush(self):
        self.f.flush()
