"""numpy specification of the device PNG encoder's LZ77 mode (tg_png_encode_lz_u8 must equal it
byte for byte).

File layout, filtering, the segmentation into SEG bytes that ignores rows, Adler-32, CRC-32 and capacity are
tests/png_ref.py's.  Only a segment's deflate differs: the segment is its own window (no match reaches across a cut),
matches come from the up to K nearest earlier positions with the same 16-bit hash of their four bytes, the parse is
greedy, and a segment is written as the smallest of three candidates -- one stored block, png_ref's Huffman-only
block, the LZ block -- the earlier one winning a tie.
"""
import bisect
import heapq
import struct
import zlib

import numpy as np

from tests.png_ref import (CLC_ORDER, FILTERS, SEG, SIGNATURE, _pack, _reverse, _smooth, canonical_codes,  # noqa: F401
                           capacity, chunk, chunks, deep_tree_frame, filtered_stream)
from tests import png_ref as P

K = 4                       # candidates per position
MIN_MATCH, MAX_MATCH = 4, 258
FAR = 4096                  # a match of exactly MIN_MATCH bytes further away than this is rejected
ROUNDS = 15                 # pointer-doubling rounds: 2^15 steps cover a segment
N_LIT, N_DIST = 286, 30
HASH_MUL = 2654435761

LEN_BASE = np.array([3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163,
                     195, 227, 258])
LEN_EXTRA = np.array([0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0])
DIST_BASE = np.array([1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049,
                      3073, 4097, 6145, 8193, 12289, 16385, 24577])
DIST_EXTRA = np.array([0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13])


def hashes(seg):
    """hash(i) for every i with i + 4 <= n."""
    s = np.asarray(seg, np.uint8).astype(np.int64)
    if s.size < 4:
        return np.zeros(0, np.int64)
    key = s[:-3] | s[1:-2] << 8 | s[2:-1] << 16 | s[3:] << 24
    return ((key * HASH_MUL) & 0xFFFFFFFF) >> 16


def candidates(seg):
    """(cand (K, n), clen (K, n)): candidate c of position i (-1: none), nearest first, and its match length."""
    s = np.asarray(seg, np.uint8)
    n = int(s.size)
    cand, clen = np.full((K, n), -1, np.int64), np.zeros((K, n), np.int64)
    h = hashes(s)
    m = h.size
    if m == 0:
        return cand, clen
    order = np.argsort(h, kind='stable')                    # positions by hash; equal hashes keep ascending position
    hs = h[order]
    pad = np.concatenate([s, np.zeros(MAX_MATCH + 1, np.uint8)])
    for c in range(K):
        r = np.arange(c + 1, m)
        ok = hs[r] == hs[r - c - 1]
        i, j = order[r[ok]], order[r[ok] - c - 1]
        cand[c, i] = j
        cap = np.minimum(MAX_MATCH, n - i)
        ln, live = np.zeros(i.size, np.int64), np.ones(i.size, bool)
        for step in range(MAX_MATCH):
            live &= (step < cap) & (pad[i + step] == pad[j + step])
            if not live.any():
                break
            ln[live] += 1
        clen[c, i] = ln
    return cand, clen


def matches(seg):
    """(length (n,), distance (n,)): the match of every position, length 0 where there is none."""
    cand, clen = candidates(seg)
    n = cand.shape[1]
    best = np.argmax(clen, axis=0)                          # the first maximum: the nearest wins a tie
    pos = np.arange(n)
    ln, dist = clen[best, pos], pos - cand[best, pos]
    ok = (ln >= MIN_MATCH) & ~((ln == MIN_MATCH) & (dist > FAR))
    return np.where(ok, ln, 0), np.where(ok, dist, 0)


def parse(ln):
    """The greedy parse: positions at which a token starts."""
    out, i, n = [], 0, len(ln)
    while i < n:
        out.append(i)
        i += int(ln[i]) if ln[i] else 1
    return np.array(out, np.int64)


def parse_by_doubling(ln):
    """The same set by pointer doubling: next[i], ROUNDS rounds, the set reachable from 0."""
    n = len(ln)
    nxt = np.append(np.where(ln > 0, np.arange(n) + ln, np.arange(n) + 1), n)     # next[n] = n
    mark = np.zeros(n + 1, bool)
    mark[0] = True
    for _ in range(ROUNDS):
        mark[nxt[mark]] = True                              # marked: reachable within 2^round - 1 steps; now twice that
        nxt = nxt[nxt]
    return np.flatnonzero(mark[:n])


def code_lengths(counts, alphabet):
    """(lengths, halvings) by section 7i's tree rule for an alphabet of `alphabet` symbols: the key is (weight, id),
    a leaf's id is its symbol, merge step k has id alphabet + k.  One used symbol: length 1."""
    work = [int(v) for v in counts]
    assert len(work) == alphabet
    if sum(1 for v in work if v) == 1:
        return np.array([1 if v else 0 for v in work], np.int64), 0
    halvings = 0
    while True:
        heap = [(wt, s) for s, wt in enumerate(work) if wt]
        heapq.heapify(heap)
        parent, k = {}, 0
        while len(heap) > 1:
            w0, i0 = heapq.heappop(heap)
            w1, i1 = heapq.heappop(heap)
            parent[i0] = parent[i1] = alphabet + k
            heapq.heappush(heap, (w0 + w1, alphabet + k))
            k += 1
        lengths = np.zeros(alphabet, np.int64)
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


def lz_block(seg, last):
    """(bytes | None, facts) of the LZ candidate of one segment; None when the parse has no match."""
    s = np.asarray(seg, np.uint8).astype(np.int64)
    ln, dist = matches(s)
    at = parse(ln)
    tl, td = ln[at], dist[at]
    is_m = tl > 0
    facts = {'tokens': [(int(a), int(b), int(c)) for a, b, c in zip(at, tl, td)], 'matches': int(is_m.sum())}
    if not is_m.any():
        return None, facts
    lsym = np.searchsorted(LEN_BASE, tl[is_m], side='right') - 1
    dsym = np.searchsorted(DIST_BASE, td[is_m], side='right') - 1
    sym = s[at].copy()
    sym[is_m] = 257 + lsym
    lit_counts = np.bincount(sym, minlength=N_LIT)
    lit_counts[256] = 1
    dist_counts = np.bincount(dsym, minlength=N_DIST)
    ll, lit_halvings = code_lengths(lit_counts, N_LIT)
    dl, dist_halvings = code_lengths(dist_counts, N_DIST)
    facts.update(lit_halvings=lit_halvings, dist_halvings=dist_halvings, dist_used=int((dist_counts > 0).sum()))
    lrev, drev = _reverse(canonical_codes(ll), ll), _reverse(canonical_codes(dl), dl)
    hlit = max(257, int(np.flatnonzero(lit_counts)[-1]) + 1) - 257
    hdist = int(np.flatnonzero(dist_counts)[-1])
    t = len(at)
    vals, bits = np.zeros((t, 4), np.int64), np.zeros((t, 4), np.int64)       # code, length extra, distance code, extra
    vals[:, 0], bits[:, 0] = lrev[sym], ll[sym]
    vals[is_m, 1], bits[is_m, 1] = tl[is_m] - LEN_BASE[lsym], LEN_EXTRA[lsym]
    vals[is_m, 2], bits[is_m, 2] = drev[dsym], dl[dsym]
    vals[is_m, 3], bits[is_m, 3] = td[is_m] - DIST_BASE[dsym], DIST_EXTRA[dsym]
    out = _pack([(0, 1), (2, 2),                                # BFINAL 0, BTYPE 10
                 (hlit, 5), (hdist, 5), (15, 4),
                 ([0 if c >= 16 else 4 for c in CLC_ORDER], 3),
                 (_reverse(ll[:hlit + 257], 4), 4), (_reverse(dl[:hdist + 1], 4), 4),
                 (vals.reshape(-1), bits.reshape(-1)), (lrev[256], ll[256]),
                 (1 if last else 0, 1), (0, 2)])                # the empty stored block ...
    out += b'\x00\x00\xff\xff'                                # ... behind the padding
    return out, facts


def deflate_segment(seg, last):
    """(bytes, {'kind': 'stored' | 'dynamic' | 'lz', ...}) of one segment: the smallest of png_ref's (stored or
    Huffman-only, stored winning their tie) and the LZ block, which has to be strictly smaller."""
    data, fact = P.deflate_segment(seg, last)
    lz, lz_fact = lz_block(seg, last)
    fact = dict(fact, **lz_fact, lz_bytes=None if lz is None else len(lz), huffman_bytes=len(data))
    if lz is not None and len(lz) < len(data):
        return lz, dict(fact, kind='lz')
    return data, fact


def encode_with_facts(img, filter='adaptive'):
    """(file bytes, {'filtered': bytes, 'types': (H,), 'segments': [{'kind', ...}, ...]})."""
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


# ---- the cases of tests/test_png_lz_cpu.py and tests/test_hip_png_lz.py ---------------------------------------------
def _row(stream):
    """The one-row frame whose filtered stream with filter 'none' is `stream` (byte 0 is the filter type 0)."""
    stream = np.asarray(stream, np.uint8)
    assert stream[0] == 0 and (stream.size - 1) % 3 == 0
    return stream[1:].reshape(1, -1, 3)


def _noise_with_tail(rs, plant):
    """A stream of 12001 noise bytes, `plant`ed, followed by a copy of its bytes 6000..8001: the copy makes the LZ
    block the smallest candidate, so what the plant does to the parse shows in the file."""
    s = rs.randint(0, 256, 12001).astype(np.uint8)
    s[0] = 0
    plant(s)
    return np.concatenate([s, s[6000:8001]])


def _search(build, accept):
    """The first seed whose stream `accept`s (an AssertionError rejects it): a seeded search, the same on every run."""
    for seed in range(64):
        try:
            s = build(np.random.RandomState(1000 + seed))
            accept(s)
        except AssertionError:
            continue
        return s
    raise AssertionError('png_lz_ref: no seed gives the case')


def _tokens(s):
    return {(a, b, c) for a, b, c in lz_block(s, True)[1]['tokens'] if b}


def repeat4_stream(distance):
    """(h) one planted 4-byte repeat at `distance`: bytes 100..104 again at 100 + distance, their neighbours differ."""
    p, q = 100, 100 + distance

    def plant(s):
        s[q:q + 4] = s[p:p + 4]
        s[q + 4], s[q - 1] = s[p + 4] ^ 0x55, s[p - 1] ^ 0x55

    def accept(s):
        cand, clen = candidates(s)
        assert cand[0, q] == p and clen[0, q] == 4 and cand[1, q] == -1
        ln, _ = matches(s[:12001])
        assert (ln > 0).sum() == (1 if distance <= FAR else 0)          # nothing but the plant in the noise
        assert ((q, 4, distance) in _tokens(s)) == (distance <= FAR)
        assert deflate_segment(s, True)[1]['kind'] == 'lz'
    return _search(lambda rs: _noise_with_tail(rs, plant), accept)


def second_nearest_stream():
    """(i) eight bytes at 200, their first four and another byte at 700, the eight again at 1500: the nearest candidate
    of 1500 gives 4, the second nearest 8."""
    def plant(s):
        s[700:704] = s[200:204]
        s[704] = s[204] ^ 0x55
        s[1500:1508] = s[200:208]
        s[1508], s[1499], s[699] = s[208] ^ 0x55, s[199] ^ 0x55, s[199] ^ 0xAA

    def accept(s):
        cand, clen = candidates(s)
        assert cand[:2, 1500].tolist() == [700, 200] and clen[:2, 1500].tolist() == [4, 8] and cand[2, 1500] == -1
        assert (1500, 8, 1300) in _tokens(s) and (700, 4, 500) in _tokens(s)
        assert deflate_segment(s, True)[1]['kind'] == 'lz'
    return _search(lambda rs: _noise_with_tail(rs, plant), accept)


def collision_stream():
    """(k) two different keys with equal hash at 300 and 900: a candidate, and no match."""
    rs = np.random.RandomState(11)
    seen = {}
    while True:
        key = rs.randint(0, 256, 4).astype(np.uint8)
        h = int(hashes(key)[0])
        if h in seen and seen[h] != key.tobytes():
            a, b = np.frombuffer(seen[h], np.uint8), key
            break
        seen[h] = key.tobytes()

    def plant(s):
        s[300:304], s[900:904] = a, b

    def accept(s):
        cand, clen = candidates(s)
        assert cand[0, 900] == 300 and clen[0, 900] < 4 and cand[1, 900] == -1
        assert not any(at == 900 for at, _, _ in _tokens(s))
        assert deflate_segment(s, True)[1]['kind'] == 'lz'
    return _search(lambda rs_: _noise_with_tail(rs_, plant), accept)


DEEP_COUNTS = [1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597]     # w[k + 2] = w[0] + .. + w[k] + 1
DEEP_CODES = [12, 11, 10, 9, 8, 7, 6, 5, 4, 18, 20, 22, 24, 25, 26, 27, 28]             # the distance symbol of each count
DEEP_NOISE = 5600                                                                       # bytes before the far matches


def deep_distance_stream():
    """A distance histogram deeper than 15 in a segment whose LZ block wins: 4180 matches of 5 bytes over 17 distance
    symbols with the counts DEEP_COUNTS (the least counts whose tree puts two leaves at depth 16).  Every match copies
    five bytes of noise that no other match copies, at the least distance of its symbol that offers such bytes, and
    the byte behind it differs from the byte behind its source, so the greedy parse takes exactly these matches.
    The nine rare symbols are near ones: their noise is laid down right in front of the copy.  The eight frequent ones
    are far ones and copy out of the first DEEP_NOISE bytes, each symbol while its distances still reach them."""
    def build(rs):
        s = np.zeros(SEG, np.uint8)
        fresh = np.zeros(SEG, bool)
        owner = {}                                            # source position -> where its copy went
        n, avoid = 1, -1                                      # the filter byte; the next byte must differ from `avoid`

        def noise(k):
            nonlocal n, avoid
            for _ in range(k):
                v = int(rs.randint(0, 256))
                while v == avoid:
                    v = int(rs.randint(0, 256))
                s[n], fresh[n], n, avoid = v, True, n + 1, -1

        def copy(i):
            nonlocal n, avoid
            d = n - i
            owner[i] = n
            for k in range(5):
                s[n + k] = s[i + k]                           # (one by one: the source may reach into the copy)
            n += 5
            avoid = int(s[n - d])

        chain, hashed = {}, 0                                 # hash -> its positions so far, ascending

        def nearer(i):
            """How many positions behind i share the hash of the four bytes at i: the candidates in front of i; K
            if one of them would match as long as i does."""
            nonlocal hashed
            if n - 3 > hashed:
                for p, h in enumerate(hashes(s[hashed:n]).tolist(), hashed):
                    chain.setdefault(h, []).append(p)
                hashed = n - 3
            lst = chain[int(hashes(s[i:i + 4])[0])]
            first = bisect.bisect_right(lst, i)
            s[n:n + 5] = s[i:i + 5]             # (as the copy would stand: a candidate may reach into it)
            if any(s[p:p + 5].tobytes() == s[i:i + 5].tobytes() for p in lst[first:]):
                return K                        # the five bytes stand nearer as well, by chance: as bad as no candidate
            return len(lst) - first

        for count, code in zip(DEEP_COUNTS[:9], DEEP_CODES[:9]):
            for _ in range(count):
                noise(int(DIST_BASE[code]))
                copy(n - int(DIST_BASE[code]))
        noise(DEEP_NOISE - n)
        whole = np.convolve(fresh[:n].astype(np.int64), np.ones(5, np.int64))[4:] == 5       # five bytes of noise from i on
        for count, code in zip(DEEP_COUNTS[9:], DEEP_CODES[9:]):
            lo, hi = int(DIST_BASE[code]), int(DIST_BASE[code + 1]) - 1
            for _ in range(count):
                first, last = max(1, n - hi), min(n - lo, whole.size - 1)
                assert first <= last
                ok = whole[first:last + 1] & (s[first:last + 1] != avoid)
                for i in first + np.flatnonzero(ok)[::-1]:                  # the least distance first
                    i = int(i)
                    if i in owner:
                        continue
                    q = owner.get(i - 1)        # that copy holds our four key bytes too: its fifth must not be ours
                    if q is not None and int(s[q + 5] if q + 5 < n else s[i]) == int(s[i + 4]):
                        continue
                    if nearer(i) >= K:          # the source would not be among the K candidates
                        continue
                    copy(i)
                    break
                else:
                    raise AssertionError('no source left: code %d, n %d' % (code, n))
        noise((1 - n) % 3)
        return s[:n].copy()

    def accept(s):
        f = deflate_segment(s, True)[1]
        assert f['kind'] == 'lz' and f['dist_halvings'] >= 1 and f['dist_used'] == 17 and f['matches'] == sum(DEEP_COUNTS)
    return _search(build, accept)


def cases():
    """[(name, frame, filter)]; tests/test_png_lz_cpu.py asserts the branch each one takes."""
    rs = np.random.RandomState(17)
    rows4 = np.repeat(rs.randint(0, 256, (1, 1400, 3)), 4, axis=0).astype(np.uint8)
    rows2 = np.repeat(rs.randint(0, 256, (1, 8200, 3)), 2, axis=0).astype(np.uint8)
    out = [(name, img, 'adaptive') for name, img in P.cases() if name != 'deep tree']
    out += [('deep tree', deep_tree_frame(), 'none'),                        # (c) an LZ block, and Huffman-only wins
            ('1x400 constant', np.full((1, 400, 3), 9, np.uint8), 'none'),   # (d) the 258 cap, the n - i cap, symbol 285
            ('64x176 zeros', np.zeros((64, 176, 3), np.uint8), 'adaptive'),  # (e) a run cut by the segment border
            ('4 rows of 1400', rows4, 'none'),                               # (f) distance 4201
            ('2 rows of 8200', rows2, 'none'),                               # (g) distance 24601, code 29
            ('repeat4 at 5000', _row(repeat4_stream(5000)), 'none'),         # (h) rejected ...
            ('repeat4 at 4000', _row(repeat4_stream(4000)), 'none'),         # ... and taken
            ('second nearest', _row(second_nearest_stream()), 'none'),       # (i)
            ('pixel 1 2 3', np.tile(np.array([1, 2, 3], np.uint8), (2, 50, 1)), 'none'),     # (j) distance 3
            ('hash collision', _row(collision_stream()), 'none'),            # (k)
            ('deep distances', _row(deep_distance_stream()), 'none')]        # the halving loop of the distance tree
    return out
