"""YUV4MPEG2 (y4m) streams of 4:2:0 frames, 8 bits per sample and on request 10 or 12: the pipe format that joins a codec
to the stream,
`ffmpeg -i in.mp4 -f yuv4mpegpipe - | python -m tecogan_pytorch_amd.main --mode infer --input - --output - | ffmpeg -i - out.mp4`.

A stream is one header line `YUV4MPEG2 W<w> H<h> F<n:d> I<p> A<n:d> C<colourspace> X<comment>...`, then per frame a line
`FRAME[ parameters]` followed by exactly frame_bytes bytes of I420 (Y, U, V planes, tightly packed).  Only progressive
8-bit 4:2:0 with a chroma siting the device kernels implement is taken: C420jpeg (centred), C420mpeg2
(left), and bare C420 or no C tag, which both mean centred per the format.  Everything else is refused by name.
A reader opened with depths=(8, 10, 12) also takes C420p10 and C420p12: samples are 16-bit
little-endian words, a frame has twice the bytes, and the tag says nothing about the siting.
A reader opened with chromas=('420', '422', '444') also takes C422 and C444 and, per allowed depth, C422p10, C422p12,
C444p10 and C444p12: the chroma planes are ceil(h/sy) x ceil(w/sx) with (sx, sy) = (2,1) / (1,1),
and none of these tags carries a siting."""
import numpy as np

MAGIC = b'YUV4MPEG2'
SITING_OF_TAG = {'420jpeg': 'center', '420mpeg2': 'left', '420': 'center'}
DEPTH_OF_TAG = {'420p10': 10, '420p12': 12}      # taken only by a reader that was opened for that depth; no siting
# taken only by a reader that was opened for that layout (and depth); no siting
PLANAR_OF_TAG = {c + sfx: (c, d) for c in ('422', '444') for sfx, d in (('', 8), ('p10', 10), ('p12', 12))}
SUBSAMPLING = {'420': (2, 2), '422': (2, 1), '444': (1, 1)}         # chroma -> (sx, sy)
TAG_OF_SITING = {'center': '420jpeg', 'left': '420mpeg2'}
MAX_LINE = 4096          # a header or FRAME line longer than this is not y4m


class Y4MError(ValueError):
    pass


def _read_line(f, limit=MAX_LINE):
    """Bytes up to (not including) the next newline; None at a clean end of the stream.  Byte by byte through a
    pipe would be slow, so readline is used where the object has it."""
    line = f.readline(limit + 1) if hasattr(f, 'readline') else None
    if line is None:
        buf = bytearray()
        while len(buf) <= limit:
            c = f.read(1)
            if not c:
                break
            buf += c
            if c == b'\n':
                break
        line = bytes(buf)
    if not line:
        return None
    if not line.endswith(b'\n'):
        raise Y4MError('y4m: a line of %d bytes without a newline (truncated stream, or not y4m)' % len(line))
    return line[:-1]


def _refusal(v, depths, chromas):
    """Why a reader opened for more than 4:2:0 refuses the C tag `v`, and what it takes."""
    why = ('no chroma planes' if v.startswith('mono') else '4:1:1' if v.startswith('411') else
           'an alpha plane' if 'alpha' in v else
           'more than 12 bits per sample' if any(b in v for b in ('p14', 'p16')) else
           'PAL-DV chroma siting' if v == '420paldv' else
           'a depth the reader was not opened for' if v in PLANAR_OF_TAG or v in DEPTH_OF_TAG else
           'a layout the reader was not opened for' if v[:3] in SUBSAMPLING else 'unknown colourspace')
    ok = ['C420jpeg', 'C420mpeg2', 'C420'] + [f'C{t}' for t, d in DEPTH_OF_TAG.items() if d in depths]
    ok += [f'C{t}' for t, (c, d) in PLANAR_OF_TAG.items() if c in chromas and d in depths]
    return Y4MError(f'y4m: C{v}: {why} (supported: {", ".join(ok)})')


def parse_header(line, depths=(8,), chromas=('420',), interlaced=False):
    """The header line (bytes, without the newline) -> dict(w, h, tags, siting, full_range, depth, chroma, interlace).  `tags` keeps the F,
    A, C and X tags as written, for the writer; full_range is True / False from XCOLORRANGE, None when the header has
    none.  depths: the bits per sample the caller takes; C420p10 / C420p12 are accepted only when theirs is among them,
    and then siting is None (the tag carries none).  chromas: the layouts the caller takes; with '422' / '444' among
    them C422 / C444 and their p10 / p12 forms (per allowed depth) are accepted, chroma says which, siting is None.  With
    the default every header is accepted or refused as a 4:2:0-only reader does.  interlaced=True: It (top field first)
    and Ib (bottom field first) are taken as well and `interlace` is 't' | 'b' | 'p' (DESIGN.md section 7o); Im (mixed)
    stays refused.  With the default anything but Ip is refused and `interlace` is 'p'."""
    depths, chromas = tuple(depths), tuple(chromas)
    interlace = 'p'
    parts = line.decode('ascii', 'replace').split(' ')
    if parts[0] != MAGIC.decode():
        raise Y4MError('y4m: the stream does not start with YUV4MPEG2')
    w = h = None
    tags, ctag, full, depth, chroma = [], None, None, 8, '420'
    for p in parts[1:]:
        if not p:
            continue
        k, v = p[0], p[1:]
        if k == 'W':
            w = int(v)
        elif k == 'H':
            h = int(v)
        elif k == 'I':
            if interlaced and v in ('t', 'b'):
                interlace = v
            elif interlaced and v == 'm':
                raise Y4MError('y4m: Im: mixed progressive and interlaced material is not supported (Ip, It or Ib)')
            elif v != 'p':
                raise Y4MError(f'y4m: I{v}: interlaced material is not supported (progressive Ip only)')
        elif k == 'C':
            planar = PLANAR_OF_TAG.get(v)
            if planar is not None and planar[0] in chromas and planar[1] in depths:
                chroma, depth = planar
            elif DEPTH_OF_TAG.get(v) in tuple(depths):
                depth = DEPTH_OF_TAG[v]
            elif v not in SITING_OF_TAG and chromas != ('420',):
                raise _refusal(v, depths, chromas)
            elif v not in SITING_OF_TAG:
                why = ('more than 8 bits per sample' if any(b in v for b in ('p10', 'p12', 'p14', 'p16')) else
                       'PAL-DV chroma siting' if v == '420paldv' else 'not 4:2:0' if not v.startswith('420') else
                       'unknown 4:2:0 variant')
                more = ''.join(f', C{t}' for t, d in DEPTH_OF_TAG.items() if d in tuple(depths))
                raise Y4MError(f'y4m: C{v}: {why} (supported: C420jpeg, C420mpeg2, C420{more})')
            ctag = v
            tags.append(p)
        elif k in 'FA':
            tags.append(p)
        elif k == 'X':
            if v.startswith('COLORRANGE='):
                r = v[len('COLORRANGE='):]
                if r not in ('FULL', 'LIMITED'):
                    raise Y4MError(f'y4m: X{v}: the range is FULL or LIMITED')
                full = r == 'FULL'
            tags.append(p)
        else:
            raise Y4MError(f'y4m: unknown header tag {p!r}')
    if w is None or h is None or w < 2 or h < 2:
        raise Y4MError(f'y4m: the header needs W and H of at least 2 (got W={w} H={h})')
    if 8 not in tuple(depths) and depth == 8:
        raise Y4MError(f'y4m: C{ctag or "420"}: 8 bits per sample, and the reader was opened for {tuple(depths)}')
    if chroma not in chromas:
        raise Y4MError(f'y4m: C{ctag or "420"}: 4:2:0, and the reader was opened for {chromas}')
    return {'w': w, 'h': h, 'tags': tags,
            'siting': SITING_OF_TAG[ctag or '420'] if depth == 8 and chroma == '420' else None,
            'full_range': full, 'depth': depth, 'chroma': chroma, 'interlace': interlace}


def frame_bytes(h, w, depth=8, chroma='420'):
    sx, sy = SUBSAMPLING[chroma]
    return (h * w + 2 * ((h + sy - 1) // sy) * ((w + sx - 1) // sx)) * (2 if depth > 8 else 1)


class Y4MReader:
    """Frames of a y4m stream, lazily: iterating yields ONE reused (frame_bytes,) uint8 numpy buffer per frame (copy
    what you keep; FRNet.infer_stream copies an item when it pulls it).  fileobj: anything with read / readinto --
    a file, sys.stdin.buffer, the read end of a pipe.  Short reads are looped over; the end of the stream inside a
    frame is an error, at a frame boundary it ends the iteration.  depths: the bits per sample that are taken, (8,) by
    default; with (8, 10, 12) C420p10 and C420p12 streams are read too -- .depth says which, .siting is None for them
    and a frame is the file's bytes, two per sample.  chromas: the layouts that are taken, ('420',) by default; with
    ('420', '422', '444') C422 / C444 streams (and their p10 / p12 forms, per depth) are read too -- .chroma says which,
    .siting is None for them.  interlaced=True: It and Ib streams are read too -- .interlace is 't' | 'b' | 'p', and a
    frame holds two fields (FRNet.infer_stream(deinterlace=...) takes them); by default they are refused."""

    def __init__(self, fileobj, depths=(8,), chromas=('420',), interlaced=False):
        self.f = fileobj
        line = _read_line(fileobj)
        if line is None:
            raise Y4MError('y4m: empty stream')
        self.header = parse_header(line, depths, chromas, interlaced)
        self.w, self.h = self.header['w'], self.header['h']
        self.siting, self.full_range, self.depth = self.header['siting'], self.header['full_range'], self.header['depth']
        self.chroma, self.interlace = self.header['chroma'], self.header['interlace']
        self.frame_bytes = frame_bytes(self.h, self.w, self.depth, self.chroma)
        self.frames_read = 0
        self._buf = np.empty(self.frame_bytes, np.uint8)

    def _fill(self, view):
        got, n = 0, len(view)
        readinto = getattr(self.f, 'readinto', None)
        while got < n:
            if readinto is not None:
                k = readinto(view[got:])
            else:
                piece = self.f.read(n - got)
                k = len(piece)
                view[got:got + k] = piece
            if not k:
                raise Y4MError(f'y4m: the stream ends inside frame {self.frames_read}: {got} of {n} bytes')
            got += k

    def __iter__(self):
        return self

    def __next__(self):
        line = _read_line(self.f)
        if line is None:
            raise StopIteration
        if line != b'FRAME' and not line.startswith(b'FRAME '):
            raise Y4MError(f'y4m: frame {self.frames_read}: expected a FRAME line, got {line[:32]!r}')
        self._fill(memoryview(self._buf))
        self.frames_read += 1
        return self._buf


def scale_rate_tag(tag, num, den):
    """The F tag `Fn:d` (frames per second) times num / den, reduced.  F0:0 (unknown) stays as it is."""
    import math
    try:
        n, d = (int(v) for v in tag[1:].split(':'))
    except ValueError:
        raise Y4MError(f'y4m: {tag!r}: the frame rate is Fn:d') from None
    if num < 1 or den < 1:
        raise Y4MError(f'y4m: the frame rate is scaled by a positive fraction, got {num}/{den}')
    if n <= 0 or d <= 0:
        return tag
    n, d = n * num, d * den
    g = math.gcd(n, d)
    return f'F{n // g}:{d // g}'


def scale_aspect_tag(tag, num, den):
    """The A tag `An:d` (pixel aspect ratio) times num / den, reduced.  A0:0 (unknown) stays as it is."""
    import math
    try:
        n, d = (int(v) for v in tag[1:].split(':'))
    except ValueError:
        raise Y4MError(f'y4m: {tag!r}: the pixel aspect ratio is An:d') from None
    if num < 1 or den < 1:
        raise Y4MError(f'y4m: the pixel aspect ratio is scaled by a positive fraction, got {num}/{den}')
    if n <= 0 or d <= 0:
        return tag
    n, d = n * num, d * den
    g = math.gcd(n, d)
    return f'A{n // g}:{d // g}'


class Y4MWriter:
    """Writes frames of W x H after a header that carries the F, A, C and X tags of `header_of_input` (a Y4MReader's
    .header, or None: C420jpeg and nothing else), then Ip.  aspect_scale (num, den): the frames were stretched, every
    pixel is num / den times as wide for its height as the input's, and the A tag is rewritten accordingly
    (scale_aspect_tag); a header without an A tag gets none.  depth 10 | 12: frames of 16-bit little-endian samples; the
    C tag becomes C420p10 / C420p12 in place of the input's, with XYSCSS=420P10 / 420P12 (the form ffmpeg writes and
    reads) in place of the input's XYSCSS.  depth 8 after a 10- or 12-bit input: the C tag (and an XYSCSS tag) of
    `siting` ('center' | 'left') in place of the input's; otherwise the input's tags as they are.  chroma '422' | '444':
    frames of that layout; the C tag becomes C422 / C444 (C422p10 ... above 8 bits) with its upper-cased XYSCSS twin
    (XYSCSS=422, 444P10, ...: the form ffmpeg is remembered to write; not verified against an ffmpeg build).  chroma
    None | '420' after a 4:2:2 or 4:4:4 input: the 8-bit C tag is the one of `siting`, as after a 10- or 12-bit input.
    rate_scale (num, den): the stream has num / den times the input's frames per second (2, 1 after deinterlacing at
    field rate) and the F tag is rewritten accordingly (scale_rate_tag); a header without an F tag gets none.  The
    writer writes Ip whatever the input was: deinterlaced frames are progressive."""

    def __init__(self, fileobj, W, H, header_of_input=None, aspect_scale=None, depth=8, siting=None, chroma=None,
                 rate_scale=None):
        if W < 2 or H < 2:
            raise Y4MError(f'y4m: W={W} H={H}')
        if depth not in (8, 10, 12):
            raise Y4MError(f'y4m: depth is 8, 10 or 12, got {depth!r}')
        chroma = '420' if chroma is None else chroma
        if chroma not in SUBSAMPLING:
            raise Y4MError(f'y4m: chroma is 420, 422 or 444, got {chroma!r}')
        self.f, self.w, self.h, self.depth, self.chroma = fileobj, W, H, depth, chroma
        self.frame_bytes = frame_bytes(H, W, depth, chroma)
        tags = list(header_of_input['tags']) if header_of_input else ['C420jpeg']
        ctag, twin = None, depth > 8 or chroma != '420'          # twin: the XYSCSS tag is written even where the input had none
        if chroma != '420':
            ctag = chroma + ('p%d' % depth if depth > 8 else '')
        elif depth > 8:
            ctag = '420p%d' % depth
        elif header_of_input and header_of_input.get('depth', 8) > 8:
            if siting not in TAG_OF_SITING:
                raise Y4MError(f'y4m: an 8-bit stream after a {header_of_input["depth"]}-bit one needs the siting for its '
                               f'C tag (center | left), got {siting!r}')
            ctag = TAG_OF_SITING[siting]
        elif header_of_input and header_of_input.get('chroma', '420') != '420':
            if siting not in TAG_OF_SITING:
                raise Y4MError(f'y4m: an 8-bit 4:2:0 stream after a C{header_of_input["chroma"]} one needs the siting for '
                               f'its C tag (center | left), got {siting!r}')
            ctag = TAG_OF_SITING[siting]
        if ctag is not None:
            had_c = any(t.startswith('C') for t in tags)
            tags = ['C' + ctag if t.startswith('C') else 'XYSCSS=' + ctag.upper() if t.startswith('XYSCSS=') else t
                    for t in tags]
            if not had_c:
                tags.append('C' + ctag)
            if 'XYSCSS=' + ctag.upper() not in tags and twin:
                tags.insert(1 + max(i for i, t in enumerate(tags) if t.startswith('C')), 'XYSCSS=' + ctag.upper())
        if aspect_scale is not None:
            tags = [scale_aspect_tag(t, *aspect_scale) if t.startswith('A') else t for t in tags]
        if rate_scale is not None:
            tags = [scale_rate_tag(t, *rate_scale) if t.startswith('F') else t for t in tags]
        self._write_all((' '.join(['YUV4MPEG2', f'W{W}', f'H{H}'] + tags + ['Ip']) + '\n').encode('ascii'))

    def _write_all(self, data):
        view = memoryview(data)
        while len(view):                            # (an unbuffered pipe may take less than it is given)
            k = self.f.write(view)
            view = view[len(view) if k is None else k:]

    def write(self, frame):
        """One I420 frame: any contiguous buffer of frame_bytes bytes (uint8, or uint16 samples above 8 bits)."""
        view = memoryview(np.ascontiguousarray(frame)).cast('B')
        if len(view) != self.frame_bytes:
            raise Y4MError(f'y4m: a {self.w}x{self.h} frame has {self.frame_bytes} bytes, got {len(view)}')
        self._write_all(b'FRAME\n')
        self._write_all(view)

    def flush(self):
        self.f.flush()
