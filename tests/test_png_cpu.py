"""The specification of the device PNG encoder itself (no GPU): tests/png_ref.py writes files
that Pillow and zlib accept, every checksum is zlib's, and every case takes the branch it was built for.  Plus the
argument checks of Png, of png= together with yuv=, and of --png-encoder."""
import io
import struct
import zlib

import numpy as np
import pytest
from PIL import Image

from tests import png_ref as P
from tecogan_pytorch_amd import main as M
from tecogan_pytorch_amd.models.networks import Png, Yuv420
from tecogan_pytorch_amd.models.networks import tecogan_nets as N

CASES = P.cases()


@pytest.mark.parametrize('filter', P.FILTERS)
@pytest.mark.parametrize('name,img', CASES, ids=[c[0] for c in CASES])
def test_files_decode_and_checksums_are_zlibs(name, img, filter):
    png, facts = P.encode_with_facts(img, filter)
    assert png == P.encode(img, filter) and len(png) <= P.capacity(*img.shape[:2])
    with Image.open(io.BytesIO(png)) as im:
        assert im.mode == 'RGB' and np.array_equal(np.asarray(im), img)
    chunks = P.chunks(png)
    assert [c[0] for c in chunks] == [b'IHDR', b'IDAT', b'IEND']
    for kind, data, crc in chunks:
        assert crc == zlib.crc32(kind + data)
    assert chunks[0][1] == struct.pack('>IIBBBBB', img.shape[1], img.shape[0], 8, 2, 0, 0, 0)
    idat = chunks[1][1]
    assert idat[:2] == b'\x78\x01'
    assert zlib.decompress(idat) == facts['filtered']
    assert struct.unpack('>I', idat[-4:])[0] == zlib.adler32(facts['filtered'])
    assert len(facts['filtered']) == img.shape[0] * (1 + 3 * img.shape[1])
    assert len(facts['segments']) == -(-len(facts['filtered']) // P.SEG)
    if filter == 'none':
        assert not facts['types'].any()


def _facts(name, filter):
    img = dict(CASES)[name]
    return img, P.encode_with_facts(img, filter)[1]


@pytest.mark.parametrize('filter', P.FILTERS)
def test_every_case_takes_its_branch(filter):
    kinds = lambda f: [s['kind'] for s in f['segments']]
    _, f = _facts('1x1', filter)
    assert kinds(f) == ['stored'] and len(f['filtered']) == 4
    _, f = _facts('8x8 constant', filter)                        # byte 0 and the end-of-block symbol: a tree of two
    assert kinds(f) == ['dynamic'] and set(f['filtered']) == {0}
    img, f = _facts('64x176 smooth', filter)                     # two segments, the second short, a row across the cut
    assert len(f['segments']) == 2 and 0 < len(f['filtered']) - P.SEG < P.SEG and P.SEG % (1 + 3 * 176) != 0
    assert kinds(f)[0] == 'dynamic'
    _, f = _facts('40x60 noise', filter)
    assert kinds(f) == ['stored'] and len(f['filtered']) > 7000
    _, f = _facts('128x85 smooth', filter)                       # exactly one full segment
    assert len(f['filtered']) == P.SEG and len(f['segments']) == 1
    _, f = _facts('129x85 smooth', filter)                       # ... and one row more
    assert len(f['filtered']) == P.SEG + 256 and len(f['segments']) == 2
    if filter == 'adaptive':
        assert len(set(_facts('40x60 noise', filter)[1]['types'].tolist())) > 1
        assert set(_facts('64x176 smooth', filter)[1]['types'].tolist()) - {0}


def test_the_deep_tree_frame_is_halved_exactly_once():
    img, f = _facts('deep tree', 'none')
    assert img.shape == (1, 9552, 3)
    counts = np.bincount(np.frombuffer(f['filtered'], np.uint8), minlength=257)
    counts[256] = 1
    used = sorted(int(c) for c in counts if c)
    assert used[:6] == [1, 1, 2, 3, 5, 8] and len(used) == 21 and used[-1] == 10948
    assert f['segments'] == [{'kind': 'dynamic', 'halvings': 1}]
    lengths = P.code_lengths(counts)[0]                          # a complete prefix code within 15 bits
    assert lengths.max() <= 15 and sum(2.0 ** -int(l) for l in lengths if l) == 1.0


def test_adaptive_picks_the_lowest_type_on_a_tie_and_the_smallest_cost():
    img = np.zeros((3, 5, 3), np.uint8)                          # every type costs 0: None wins
    assert P.filtered_stream(img)[1].tolist() == [0, 0, 0]
    img[:] = 200                                                 # row 0: Sub (first pixel only); later rows: Up is free
    assert P.filtered_stream(img)[1].tolist() == [1, 2, 2]
    stream, types = P.filtered_stream(dict(CASES)['64x176 smooth'])
    assert np.array_equal(stream.reshape(64, -1)[:, 0], types)


def test_canonical_codes_are_rfc1951s_example():
    assert P.canonical_codes(np.array([3, 3, 3, 3, 3, 2, 4, 4])).tolist() == [2, 3, 4, 5, 6, 0, 14, 15]


def test_capacity_is_the_all_stored_size():
    rs = np.random.RandomState(0)
    for h, w in ((1, 1), (40, 60), (128, 85), (129, 85)):
        img = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
        png, facts = P.encode_with_facts(img, 'none')
        assert all(s['kind'] == 'stored' for s in facts['segments']) and len(png) == P.capacity(h, w)


# ---------------------------------------------------------------- the Python surface's argument checks
def test_png_validation():
    spec = Png()
    assert spec.filter == 'adaptive' and Png('none').filter == 'none' and spec.code() == 1 and Png('none').code() == 0
    assert spec == Png('adaptive') and spec != Png('none') and hash(spec) == hash(Png()) and 'adaptive' in repr(spec)
    with pytest.raises(AttributeError):
        spec.filter = 'none'
    with pytest.raises(AttributeError):
        del spec.filter
    for bad in ('paeth', 0, None, b'none'):
        with pytest.raises(ValueError, match='Png'):
            Png(bad)


def test_png_with_yuv_is_refused_before_anything_is_pulled():
    net = N.FRNet(3, 3, 64, 10, 'BD', 4)
    pulled = []

    def frames():
        pulled.append(1)
        yield np.zeros((8, 8, 3), np.uint8)

    with pytest.raises(ValueError, match='png and yuv'):
        net.infer_stream(frames(), device='cpu', yuv=Yuv420(8, 8), png=Png())
    with pytest.raises(ValueError, match='Png'):
        net.infer_stream(frames(), device='cpu', png='adaptive')
    assert not pulled
    assert list(net.infer_stream(iter([]), device='cpu', png=Png())) == []


def test_png_encoder_option(tmp_path, capsys):
    assert M.parse_args(['--mode', 'infer']).png_encoder == 'pillow'
    folder = str(tmp_path)
    assert M.parse_args(['--mode', 'infer', '--input', folder, '--png-encoder', 'device']).png_encoder == 'device'
    y4m = tmp_path / 'clip.y4m'
    y4m.write_bytes(b'YUV4MPEG2 W2 H2 F25:1\n')
    for src in (str(y4m), '-'):
        with pytest.raises(SystemExit) as e:
            M.parse_args(['--mode', 'infer', '--input', src, '--output', '-', '--png-encoder', 'device'])
        assert e.value.code == 2 and 'y4m' in capsys.readouterr().err
    with pytest.raises(SystemExit):
        M.parse_args(['--mode', 'infer', '--png-encoder', 'zlib'])
    assert M.parse_args(['--mode', 'infer', '--input', str(y4m), '--png-encoder', 'pillow']).png_encoder == 'pillow'
