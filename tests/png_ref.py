"""numpy specification of the device PNG encoder (tg_png_encode_u8 must equal it byte for byte).

A frame is (H, W, 3) uint8 RGB.  The file is signature, IHDR (8 bit, colour type 2), ONE IDAT, IEND.  The IDAT is a
zlib stream `78 01`, deflate segments, Adler-32.  The filtered stream (H rows of 1 + 3W bytes) is cut into segments of
SEG bytes, the cut ignores rows; every segment is deflated on its own, Huffman only (no LZ77 matches), as one dynamic
block followed by an empty stored block that restores byte alignment, or as one stored block when that is not larger.
"""
import heapq
import struct
import zlib

import numpy as np

SEG = 32768
SIGNATURE = b'\x89PNG\r\n\x1a\n'
FILTERS = ('adaptive', 'none')
CLC_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
DYN_HEADER_BITS = 3 + 14 + 57 + 1032


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filtered_stream(img, filter='adaptive'):
    """(stream bytes (H * (1 + 3W),) uint8, filter type per row (H,))."""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3 or img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError(f'png_ref: a frame is (H, W, 3) uint8, got {img.dtype} {img.shape}')
    if filter not in FILTERS:
        raise ValueError(f'png_ref: filter is one of {FILTERS}, got {filter!r}')
    H, W = img.shape[:2]
    x = img.reshape(H, 3 * W).astype(np.int64)
    a = np.zeros_like(x)
    a[:, 3:] = x[:, :-3]
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[1:, 3:] = x[:-1, :-3]
    cand = np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - _paeth(a, b, c)]) & 255          # (5, H, 3W)
    if filter == 'none':
        types = np.zeros(H, np.int64)
    else:
        cost = np.where(cand >= 128, 256 - cand, cand).sum(axis=2)                              # sum |int8(byte)|
        types = np.argmin(cost, axis=0)                                                        # first minimum: lowest type
    out = np.empty((H, 1 + 3 * W), np.uint8)
    out[:, 0] = types
    out[:, 1:] = cand[types, np.arange(H)]
    return out.reshape(-1), types


def code_lengths(counts):
    """(lengths (257,), halvings) of the spec's Huffman construction for the 257 counts of one segment."""
    work = [int(v) for v in counts]
    halvings = 0
    while True:
        heap = [(wt, s) for s, wt in enumerate(work) if wt]
        heapq.heapify(heap)
        parent, k = {}, 0
        while len(heap) > 1:
            w0, i0 = heapq.heappop(heap)
            w1, i1 = heapq.heappop(heap)
            parent[i0] = parent[i1] = 257 + k
            heapq.heappush(heap, (w0 + w1, 257 + k))
            k += 1
        lengths = np.zeros(257, np.int64)
        for s, wt in enumerate(work):
            if wt:
                d, node = 0, s
                while node in parent:
                    node, d = parent[node], d + 1
                lengths[s] = d
        if lengths.max() <= 15:
            return lengths, halvings
        work = [(wt + 1) >> 1 if wt else 0 for wt in work]
        halvings += 1


def canonical_codes(lengths):
    """RFC 1951 section 3.2.2."""
    bl_count = np.bincount(lengths, minlength=16)
    bl_count[0] = 0
    next_code, code = [0] * 16, 0
    for bits in range(1, 16):
        code = (code + int(bl_count[bits - 1])) << 1
        next_code[bits] = code
    codes = np.zeros(len(lengths), np.int64)
    for s, ln in enumerate(lengths):
        if ln:
            codes[s] = next_code[ln]
            next_code[ln] += 1
    return codes


def _reverse(value, nbits):
    """The low nbits of value, bit-reversed: Huffman codes go into the LSB-first stream MSB first."""
    value, nbits = np.asarray(value, np.int64), np.asarray(nbits, np.int64)
    out = np.zeros_like(value)
    for j in range(15):
        out |= np.where(j < nbits, ((value >> j) & 1) << np.maximum(nbits - 1 - j, 0), 0)
    return out


def _pack(fields):
    """[(values, nbits)] (scalars or arrays), each value LSB first, one after the other -> bytes, zero padded."""
    vals = np.concatenate([np.broadcast_arrays(np.asarray(v, np.int64), np.asarray(n, np.int64))[0].reshape(-1)
                           for v, n in fields])
    nbits = np.concatenate([np.broadcast_arrays(np.asarray(v, np.int64), np.asarray(n, np.int64))[1].reshape(-1)
                            for v, n in fields])
    start = np.cumsum(nbits) - nbits
    bits = np.zeros(int(nbits.sum()), np.uint8)
    for j in range(int(nbits.max())):
        m = nbits > j
        bits[start[m] + j] = (vals[m] >> j) & 1
    return np.packbits(bits, bitorder='little').tobytes()


def deflate_segment(seg, last):
    """(bytes, {'kind': 'stored' | 'dynamic', 'halvings': int}) of one segment of the filtered stream."""
    seg = np.asarray(seg, np.uint8)
    n = int(seg.size)
    counts = np.bincount(seg, minlength=257)
    counts[256] = 1
    lengths, halvings = code_lengths(counts)
    dyn = (DYN_HEADER_BITS + int((counts * lengths).sum()) + 3 + 7) // 8 + 4
    if 5 + n <= dyn:
        return (bytes([1 if last else 0]) + struct.pack('<HH', n, n ^ 0xFFFF) + seg.tobytes(),
                {'kind': 'stored', 'halvings': halvings})
    rev = _reverse(canonical_codes(lengths), lengths)
    lit = np.append(lengths, 0)                                 # 257 literal lengths and one distance length
    out = _pack([(0, 1), (2, 2),                                # BFINAL 0, BTYPE 10
                 (0, 5), (0, 5), (15, 4),                       # HLIT 257, HDIST 1, HCLEN 19
                 ([0 if s >= 16 else 4 for s in CLC_ORDER], 3),
                 (_reverse(lit, 4), 4),                         # the code of a length is the length itself, 4 bits
                 (rev[seg], lengths[seg]), (rev[256], lengths[256]),
                 (1 if last else 0, 1), (0, 2)])                # the empty stored block ...
    out += b'\x00\x00\xff\xff'                                # ... behind the padding
    assert len(out) == dyn
    return out, {'kind': 'dynamic', 'halvings': halvings}


def chunk(kind, data):
    return struct.pack('>I', len(data)) + kind + data + struct.pack('>I', zlib.crc32(kind + data))


def encode_with_facts(img, filter='adaptive'):
    """(file bytes, {'filtered': bytes, 'types': (H,), 'segments': [{'kind', 'halvings'}, ...]})."""
    stream, types = filtered_stream(img, filter)
    H, W = np.asarray(img).shape[:2]
    parts, facts = [b'\x78\x01'], []
    for off in range(0, stream.size, SEG):
        data, fact = deflate_segment(stream[off:off + SEG], off + SEG >= stream.size)
        parts.append(data)
        facts.append(fact)
    raw = stream.tobytes()
    parts.append(struct.pack('>I', zlib.adler32(raw)))
    png = (SIGNATURE + chunk(b'IHDR', struct.pack('>IIBBBBB', W, H, 8, 2, 0, 0, 0)) + chunk(b'IDAT', b''.join(parts)) +
           chunk(b'IEND', b''))
    return png, {'filtered': raw, 'types': types, 'segments': facts}


def encode(img, filter='adaptive'):
    return encode_with_facts(img, filter)[0]


def capacity(h, w):
    """Bytes one encoded frame can need: every segment stored."""
    f = h * (3 * w + 1)
    return 63 + f + 5 * ((f + SEG - 1) // SEG)


def chunks(png):
    """[(type, data, crc)] of a PNG file."""
    assert png[:8] == SIGNATURE
    out, pos = [], 8
    while pos < len(png):
        n, = struct.unpack('>I', png[pos:pos + 4])
        out.append((png[pos + 4:pos + 8], png[pos + 8:pos + 8 + n], struct.unpack('>I', png[pos + 8 + n:pos + 12 + n])[0]))
        pos += 12 + n
    assert pos == len(png)
    return out


# ---- the cases of tests/test_png_cpu.py and tests/test_hip_png.py ---------------------------------------------------
def _smooth(h, w):
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([(2 * x + y) % 256, (x + 3 * y) // 2 % 256, (x * y // 16 + 40) % 256], axis=2).astype(np.uint8)


def deep_tree_frame():
    """One row, W = 9552, for filter='none': 19 byte values with Fibonacci counts 2, 3, 5, ..., 10946 (the 2 left-over
    bytes go to the most frequent value); with the filter byte and symbol 256 (count 1 each) the histogram is
    Fibonacci and the unlimited tree is deeper than 15."""
    fib = [2, 3]
    while len(fib) < 19:
        fib.append(fib[-1] + fib[-2])
    assert fib[-1] == 10946
    n = 3 * 9552
    fib[-1] += n - sum(fib)
    assert n - sum(fib) == 0 and fib[-1] == 10948
    vals = np.repeat(np.arange(1, 20, dtype=np.uint8), fib)                # value 0 is the filter byte's alone
    np.random.RandomState(7).shuffle(vals)
    return vals.reshape(1, 9552, 3)


def cases():
    """[(name, frame)]; tests/test_png_cpu.py asserts the branch each one takes."""
    rs = np.random.RandomState(3)
    return [
        ('1x1', np.array([[[7, 200, 31]]], np.uint8)),                    # stored
        ('8x8 constant', np.zeros((8, 8, 3), np.uint8)),                  # two used symbols: byte 0 and end of block
        ('64x176 smooth', _smooth(64, 176)),                              # two segments, a row across the cut
        ('40x60 noise', rs.randint(0, 256, (40, 60, 3)).astype(np.uint8)),        # stored fallback
        ('128x85 smooth', _smooth(128, 85)),                              # 256 bytes per row: exactly one segment
        ('129x85 smooth', _smooth(129, 85)),                              # ... and one row
        ('deep tree', deep_tree_frame()),                                 # the length-limit loop (filter='none')
    ]
