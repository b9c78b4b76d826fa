"""The specification of the device PNG encoder's LZ77 mode itself (no GPU): tests/png_lz_ref.py
writes files that Pillow and zlib accept, never longer than tests/png_ref.py's, every case takes the branch it was
built for, and the pointer-doubling restatement of the parse equals the sequential one.  Plus the two new symbols of
the C ABI and the argument checks of Png(lz77=...) and --png-lz77."""
import ctypes
import io
import zlib

import numpy as np
import pytest
from PIL import Image

from tests import png_lz_ref as Z
from tests import png_ref as P
from tecogan_pytorch_amd import _lib as L
from tecogan_pytorch_amd import main as M
from tecogan_pytorch_amd.models.networks import Png

CASES = Z.cases()
IDS = [c[0] for c in CASES]
_FACTS = {}


def facts(name):
    """(frame, file, facts) of a case, computed once."""
    if name not in _FACTS:
        _, img, filter = next(c for c in CASES if c[0] == name)
        _FACTS[name] = (img,) + Z.encode_with_facts(img, filter)
    return _FACTS[name]


def kinds(name):
    return [s['kind'] for s in facts(name)[2]['segments']]


def segments(name):
    raw = np.frombuffer(facts(name)[2]['filtered'], np.uint8)
    return [raw[off:off + P.SEG] for off in range(0, raw.size, P.SEG)]


def matches(name, k=0):
    return [(at, ln, d) for at, ln, d in facts(name)[2]['segments'][k]['tokens'] if ln]


@pytest.mark.parametrize('name,img,filter', CASES, ids=IDS)
def test_files_decode_and_are_never_longer(name, img, filter):
    _, png, f = facts(name)
    with Image.open(io.BytesIO(png)) as im:
        assert im.mode == 'RGB' and np.array_equal(np.asarray(im), img)
    chunks = P.chunks(png)
    assert [c[0] for c in chunks] == [b'IHDR', b'IDAT', b'IEND']
    for kind, data, crc in chunks:
        assert crc == zlib.crc32(kind + data)
    assert zlib.decompress(chunks[1][1]) == f['filtered'] == P.filtered_stream(img, filter)[0].tobytes()
    base = P.encode(img, filter)
    assert len(png) <= len(base) <= P.capacity(*img.shape[:2])
    if all(s['matches'] == 0 for s in f['segments']):
        assert png == base
    for s in f['segments']:
        assert (s['kind'] == 'lz') == (s['lz_bytes'] is not None and s['lz_bytes'] < s['huffman_bytes'])


@pytest.mark.parametrize('name,img,filter', CASES, ids=IDS)
def test_pointer_doubling_equals_the_sequential_parse(name, img, filter):
    for seg in segments(name):
        ln, _ = Z.matches(seg)
        seq = Z.parse(ln)
        assert np.array_equal(Z.parse_by_doubling(ln), seq)
        assert seq[0] == 0 and len(seq) <= seg.size


def test_every_case_takes_its_branch():
    assert kinds('1x1') == ['stored']
    assert kinds('40x60 noise') == ['stored'] and facts('40x60 noise')[2]['segments'][0]['matches'] == 0
    assert facts('40x60 noise')[1] == P.encode(facts('40x60 noise')[0], 'adaptive')             # today's bytes
    s, = facts('8x8 constant')[2]['segments']                    # one match, one distance symbol: the length-1 rule
    assert s['kind'] == 'lz' and s['matches'] == 1 and s['dist_used'] == 1
    assert matches('8x8 constant') == [(1, 199, 1)]
    assert kinds('64x176 smooth') == ['lz', 'lz']                # (b)
    assert kinds('128x85 smooth') == ['lz'] and kinds('129x85 smooth') == ['lz', 'lz']
    s, = facts('deep tree')[2]['segments']                       # (c) an LZ block exists and Huffman-only wins
    assert s['kind'] == 'dynamic' and s['matches'] > 0 and s['lz_bytes'] > s['huffman_bytes'] and s['halvings'] == 1
    assert facts('deep tree')[1] == P.encode(facts('deep tree')[0], 'none')
    # (d) 1201 bytes: the filter byte, a literal 9, then distance 1 at 258 (symbol 285) four times and the n - i cap
    assert kinds('1x400 constant') == ['lz']
    assert matches('1x400 constant') == [(2, 258, 1), (260, 258, 1), (518, 258, 1), (776, 258, 1), (1034, 167, 1)]
    # (e) a run of zeros cut by the segment border: the second segment starts again with a literal
    assert kinds('64x176 zeros') == ['lz', 'lz'] and len(facts('64x176 zeros')[2]['filtered']) == 64 * 529
    first, second = matches('64x176 zeros', 0), matches('64x176 zeros', 1)
    assert first[0] == (1, 258, 1) and first[-1] == (32509, 258, 1)          # 1 + 127 * 258 = 32767: one literal is left
    assert facts('64x176 zeros')[2]['segments'][0]['tokens'][-1] == (P.SEG - 1, 0, 0)
    assert second[0] == (1, 258, 1) and second[-1][1] < 258 and second[-1][0] + second[-1][1] == 64 * 529 - P.SEG
    # (f) distance 4201 = 3 * 1400 + 1: code 24, 11 extra bits would end at 6144; 4201 lies in 4097..6144
    assert kinds('4 rows of 1400') == ['lz'] and {d for _, _, d in matches('4 rows of 1400')} == {4201}
    assert int(np.searchsorted(Z.DIST_BASE, 4201, side='right')) - 1 == 24
    # (g) distance 24601: code 29, 13 extra bits; the second segment (the rest of row 2) has nothing to refer to
    assert kinds('2 rows of 8200') == ['lz', 'stored'] and {d for _, _, d in matches('2 rows of 8200')} == {24601}
    assert int(np.searchsorted(Z.DIST_BASE, 24601, side='right')) - 1 == 29 and Z.DIST_EXTRA[29] == 13
    assert facts('2 rows of 8200')[2]['segments'][1]['matches'] == 0
    # (h) the length-4 rule, both sides (the streams assert their candidates when they are built)
    assert kinds('repeat4 at 5000') == ['lz'] and kinds('repeat4 at 4000') == ['lz']
    assert (5100, 4, 5000) not in matches('repeat4 at 5000') and not any(ln == 4 for _, ln, _ in matches('repeat4 at 5000'))
    assert (4100, 4, 4000) in matches('repeat4 at 4000')
    cand, clen = Z.candidates(segments('repeat4 at 5000')[0])
    assert cand[0, 5100] == 100 and clen[0, 5100] == 4
    # (i) the second-nearest candidate is the longer one
    cand, clen = Z.candidates(segments('second nearest')[0])
    assert cand[:2, 1500].tolist() == [700, 200] and clen[:2, 1500].tolist() == [4, 8]
    assert (1500, 8, 1300) in matches('second nearest') and kinds('second nearest') == ['lz']
    # (j) distance 3: the filter byte, 1 2 3, and the pixel row as one overlapping match
    assert kinds('pixel 1 2 3') == ['lz'] and matches('pixel 1 2 3')[0] == (4, 147, 3)
    # (k) a collision is a candidate and not a match
    seg = segments('hash collision')[0]
    cand, clen = Z.candidates(seg)
    h = Z.hashes(seg)
    assert cand[0, 900] == 300 and h[900] == h[300] and seg[900:904].tobytes() != seg[300:304].tobytes()
    assert clen[0, 900] < 4 and not any(at == 900 for at, _, _ in matches('hash collision'))
    assert kinds('hash collision') == ['lz']


def test_a_distance_tree_deeper_than_15_is_halved_inside_a_winning_lz_block():
    s, = facts('deep distances')[2]['segments']
    assert s['kind'] == 'lz' and s['dist_halvings'] == 1 and s['lit_halvings'] == 0 and s['dist_used'] == 17
    toks = matches('deep distances')
    assert len(toks) == sum(Z.DEEP_COUNTS) == 4180 and {ln for _, ln, _ in toks} == {5}
    counts = np.bincount(np.searchsorted(Z.DIST_BASE, [d for _, _, d in toks], side='right') - 1, minlength=30)
    assert sorted(c for c in counts.tolist() if c) == Z.DEEP_COUNTS
    assert [int(counts[c]) for c in Z.DEEP_CODES] == Z.DEEP_COUNTS
    parent = {}                                                  # the unlimited tree: the two rarest leaves at depth 16
    import heapq
    heap = [(int(c), i) for i, c in enumerate(counts) if c]
    heapq.heapify(heap)
    k = 0
    while len(heap) > 1:
        (w0, a), (w1, b) = heapq.heappop(heap), heapq.heappop(heap)
        parent[a] = parent[b] = 30 + k
        heapq.heappush(heap, (w0 + w1, 30 + k))
        k += 1
    depth = lambda node: 0 if node not in parent else 1 + depth(parent[node])
    assert max(depth(i) for i, c in enumerate(counts) if c) == 16
    lengths, halvings = Z.code_lengths(counts, 30)
    assert halvings == 1 and lengths.max() <= 15 and sum(2.0 ** -int(l) for l in lengths if l) == 1.0


def test_symbol_tables_are_rfc1951s():
    assert len(Z.LEN_BASE) == len(Z.LEN_EXTRA) == 29 and len(Z.DIST_BASE) == len(Z.DIST_EXTRA) == 30
    assert Z.LEN_BASE[-1] == 258 and Z.LEN_EXTRA[-1] == 0
    assert all(Z.LEN_BASE[i] + (1 << Z.LEN_EXTRA[i]) == Z.LEN_BASE[i + 1] for i in range(27))
    assert Z.LEN_BASE[27] + (1 << Z.LEN_EXTRA[27]) == 259                  # 227 .. 258, 258 has its own symbol as well
    assert all(Z.DIST_BASE[i] + (1 << Z.DIST_EXTRA[i]) == Z.DIST_BASE[i + 1] for i in range(29))
    assert Z.DIST_BASE[29] + (1 << Z.DIST_EXTRA[29]) == 32769


def test_one_used_distance_symbol_gets_length_one_and_trees_stay_within_15():
    counts = np.zeros(30, np.int64)
    counts[7] = 12
    assert Z.code_lengths(counts, 30)[0].tolist() == [0] * 7 + [1] + [0] * 22
    fib = [1, 1]
    while len(fib) < 24:
        fib.append(fib[-1] + fib[-2])
    lengths, halvings = Z.code_lengths(fib + [0] * 6, 30)
    assert halvings >= 1 and lengths.max() <= 15 and sum(2.0 ** -int(l) for l in lengths if l) == 1.0
    counts = np.bincount(np.frombuffer(facts('deep tree')[2]['filtered'], np.uint8), minlength=257)
    counts[256] = 1
    assert np.array_equal(Z.code_lengths(counts, 257)[0], P.code_lengths(counts)[0])          # the same rule


# ---------------------------------------------------------------- the C ABI and the Python surface
def test_abi_declares_and_exports_the_two_symbols():
    I, I64, PTR = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    assert L.SIGNATURES['tg_png_lz_workspace_bytes'] == (I64, [I, I, I])
    res, args = L.SIGNATURES['tg_png_encode_lz_u8']
    assert res is I and args == [PTR, I, I, I, I, PTR, I64, PTR, PTR, PTR]
    assert L.SIGNATURES['tg_png_encode_lz_u8'] == L.SIGNATURES['tg_png_encode_u8']
    handle = ctypes.CDLL(L.LIB_PATH)
    assert hasattr(handle, 'tg_png_lz_workspace_bytes') and hasattr(handle, 'tg_png_encode_lz_u8')
    lib = L.lib()
    assert lib.tg_png_lz_workspace_bytes(0, 8, 8) == -1 and lib.tg_png_lz_workspace_bytes(1, 8, 0) == -1
    assert lib.tg_png_lz_workspace_bytes(1, 1 << 16, 1 << 14) == -1
    for n, h, w in ((1, 8, 8), (3, 64, 176)):                    # 256 KiB per segment on top of the Huffman-only one
        nseg = -(-h * (3 * w + 1) // P.SEG)
        extra = lib.tg_png_lz_workspace_bytes(n, h, w) - lib.tg_png_workspace_bytes(n, h, w)
        assert extra == n * nseg * 8 * P.SEG + -(-4 * n * nseg // 16) * 16
    rc = lib.tg_png_encode_lz_u8(None, 1, 8, 8, 1, None, 0, None, None, None)
    assert rc == L.TG_E_ARG and b'png_encode_lz_u8' in lib.tg_last_error_string()


def test_png_lz77_validation():
    assert Png().lz77 is False and Png(lz77=True).lz77 is True and Png('none', True).filter == 'none'
    assert Png() == Png('adaptive', False) and Png(lz77=True) != Png() and hash(Png(lz77=True)) == hash(Png('adaptive', True))
    assert 'lz77=True' in repr(Png(lz77=True))
    assert Png().entry() == ('tg_png_encode_u8', 'tg_png_workspace_bytes')
    assert Png(lz77=True).entry() == ('tg_png_encode_lz_u8', 'tg_png_lz_workspace_bytes')
    assert Png(lz77=True).code() == 1
    with pytest.raises(AttributeError):
        Png().lz77 = True
    for bad in (1, 0, 'yes', None):
        with pytest.raises(ValueError, match='Png'):
            Png(lz77=bad)


def test_ops_png_encode_refuses_an_lz77_that_is_no_bool():
    import torch
    from tecogan_pytorch_amd import ops
    for bad in (1, 0, 'yes', None):                              # (ops raises TecoganHipError for every bad argument)
        with pytest.raises(L.TecoganHipError, match='lz77'):
            ops.png_encode(torch.zeros(2, 2, 3, dtype=torch.uint8), 'adaptive', lz77=bad)


def test_png_lz77_option(tmp_path, capsys):
    folder = str(tmp_path)
    assert M.parse_args(['--mode', 'infer', '--input', folder, '--png-encoder', 'device']).png_lz77 is False
    assert M.parse_args(['--mode', 'infer', '--input', folder, '--png-encoder', 'device', '--png-lz77']).png_lz77 is True
    for extra in ([], ['--png-encoder', 'pillow']):
        with pytest.raises(SystemExit) as e:
            M.parse_args(['--mode', 'infer', '--input', folder, '--png-lz77'] + extra)
        assert e.value.code == 2 and '--png-encoder device' in capsys.readouterr().err
    with pytest.raises(ValueError, match='png_lz77'):
        M.infer({}, folder, folder, png_lz77=True)
