"""Semi-planar YUV without a device: the relayout and its inverse, the package's helpers against
the specification's, the two new fields of Yuv, the refusal of interlaced semi-planar input, the raw-video reader and
writer, the command line's refusals, and the three prototypes in the header."""
import io
import os
import re

import numpy as np
import pytest

from tecogan_pytorch_amd import semiplanar
from tests import semiplanar_ref as S
from tests import yuv_planar_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(2, 2), (3, 5), (4, 8), (9, 11), (16, 24)]
NEW = ('tg_yuv_semiplanar_to_rgb_f32', 'tg_rgb_u8_to_yuv_semiplanar', 'tg_rgb_f32_to_yuv_semiplanar16')
PLANAR = ('tg_yuv_planar_to_rgb_f32', 'tg_rgb_u8_to_yuv_planar', 'tg_rgb_f32_to_yuv_planar16')


def _planar(n, h, w, chroma, depth, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 1 << depth, (n, P.frame_samples(h, w, chroma))).astype(np.uint8 if depth == 8 else np.uint16)


@pytest.mark.parametrize('chroma', P.CHROMAS)
@pytest.mark.parametrize('depth', P.DEPTHS)
def test_relayout_round_trip_and_layout(chroma, depth):
    for h, w in SIZES:
        x = _planar(2, h, w, chroma, depth, h * 100 + w)
        semi = S.to_semi(x, h, w, chroma, depth)
        assert semi.shape == x.shape and semi.dtype == x.dtype
        assert np.array_equal(S.to_planar(semi, h, w, chroma, depth), x)
        assert np.array_equal(semiplanar.to_planar(semiplanar.to_semi(x, h, w, chroma, depth), h, w, chroma, depth), x)
        ch, cw = P.chroma_size(h, w, chroma)
        y, u, v = P.planes(x, h, w, chroma)
        sh = 0 if depth == 8 else 16 - depth
        assert np.array_equal(semi[:, :h * w] >> sh, y.reshape(2, -1))
        # sample 2c of chroma row r is U[r, c], sample 2c + 1 is V[r, c]
        rows = semi[:, h * w:].reshape(2, ch, 2 * cw) >> sh
        assert np.array_equal(rows[:, :, 0::2], u) and np.array_equal(rows[:, :, 1::2], v)
        if depth > 8:
            assert not (semi & ((1 << sh) - 1)).any()               # the low bits are zero on the way out


@pytest.mark.parametrize('depth', (10, 12))
def test_low_bits_of_a_word_are_dropped(depth):
    h, w = 6, 8
    x = _planar(1, h, w, '420', depth, 3)
    semi = S.to_semi(x, h, w, '420', depth)
    noise = np.random.default_rng(4).integers(0, 1 << (16 - depth), semi.shape).astype(np.uint16)
    assert noise.any()
    assert np.array_equal(S.to_planar(semi | noise, h, w, '420', depth), x)
    assert np.array_equal(semiplanar.to_planar(semi | noise, h, w, '420', depth), x)


@pytest.mark.parametrize('chroma', P.CHROMAS)
@pytest.mark.parametrize('depth', P.DEPTHS)
def test_package_helpers_equal_the_specification(chroma, depth):
    from tecogan_pytorch_amd.models.networks import yuv_semiplanes
    for h, w in SIZES:
        x = _planar(3, h, w, chroma, depth, h + w)
        semi = semiplanar.to_semi(x, h, w, chroma, depth)
        assert semi.dtype == x.dtype and np.array_equal(semi, S.to_semi(x, h, w, chroma, depth))
        back = semiplanar.to_planar(semi, h, w, chroma, depth)
        assert back.dtype == x.dtype and np.array_equal(back, x)
        assert np.array_equal(semiplanar.to_semi(x[0], h, w, chroma, depth), semi[0])          # a single frame
        ch, cw = P.chroma_size(h, w, chroma)
        for chunk in (semi, semi.view(np.uint8)):                   # samples, or the bytes the stream yields
            y, uv = yuv_semiplanes(chunk, h, w, chroma, depth)
            assert y.shape == (3, h, w) and uv.shape == (3, ch, cw, 2) and y.dtype == uv.dtype == semi.dtype
            assert np.array_equal(y.reshape(3, -1), semi[:, :h * w]) and np.array_equal(uv.reshape(3, -1), semi[:, h * w:])
        y, uv = yuv_semiplanes(semi[1], h, w, chroma, depth)
        assert y.shape == (h, w) and uv.shape == (ch, cw, 2)
    with pytest.raises(ValueError):
        semiplanar.to_semi(x.astype(np.int32), h, w, chroma, depth)
    with pytest.raises(ValueError):
        semiplanar.to_planar(x[:, :-1], h, w, chroma, depth)
    with pytest.raises(ValueError):
        semiplanar.to_semi(x, h, w, '411', depth)


def test_yuv_fields_are_validated_and_sizes_do_not_depend_on_the_layout():
    from tecogan_pytorch_amd.models.networks import Yuv
    a = Yuv(9, 11, '422', '444', depth=10, out_depth=12)
    b = Yuv(9, 11, '422', '444', depth=10, out_depth=12, layout='semi', out_layout='semi')
    assert (a.layout, a.out_layout, a.ol) == ('planar', None, 'planar') and (b.layout, b.ol) == ('semi', 'semi')
    assert Yuv(9, 11, layout='semi').ol == 'semi' and Yuv(9, 11, layout='semi', out_layout='planar').ol == 'planar'
    assert Yuv(9, 11, out_layout='semi').layout == 'planar'
    assert a.frame_bytes == b.frame_bytes == 2 * P.frame_samples(9, 11, '422')
    assert a.out_size_bytes(36, 44) == b.out_size_bytes(36, 44) == b.out_frame_bytes(4) == 2 * 3 * 36 * 44
    with pytest.raises(ValueError, match='even width'):
        Yuv(9, 11, out_chroma='422', out_layout='semi').out_size_bytes(36, 43)
    for bad in ('nv12', 'SEMI', None, 1, b'semi'):
        with pytest.raises(ValueError, match='layout'):
            Yuv(9, 11, layout=bad)
    for bad in ('nv12', '', 0, True):
        with pytest.raises(ValueError, match='out_layout'):
            Yuv(9, 11, out_layout=bad)
    # the fields are the last two: every positional call of before means what it meant
    import dataclasses
    assert [f.name for f in dataclasses.fields(Yuv)][-2:] == ['layout', 'out_layout']


def test_launch_tuples_follow_the_layout_per_side():
    from tecogan_pytorch_amd import _lib as L
    from tecogan_pytorch_amd.models.networks import Yuv, Yuv420
    args = (16, 24, '422', '444', 'bt2020', True, 'center')
    plain = Yuv(*args, depth=10, out_depth=12)
    codes = (L.YUV_PLANAR_MATRIX['bt2020'], 1, L.YUV_SITING['center'])
    # with the fields at their defaults the tuples are the planar ones, spelled out here
    assert plain.input_launch() == ('tg_yuv_planar_to_rgb_f32', (16, 24, L.YUV_CHROMA['422'], 10, *codes))
    assert plain.out_launch(64, 96) == ('tg_rgb_u8_to_yuv_planar', (64, 96, L.YUV_CHROMA['444'], *codes))
    assert plain.deep_launch(64, 96) == ('tg_rgb_f32_to_yuv_planar16', (64, 96, L.YUV_CHROMA['444'], 12, *codes))
    assert Yuv(*args, depth=10, out_depth=12, layout='planar', out_layout='planar').input_launch() == plain.input_launch()
    both = Yuv(*args, depth=10, out_depth=12, layout='semi')
    assert [both.input_launch()[0], both.out_launch(64, 96)[0], both.deep_launch(64, 96)[0]] == list(NEW)
    for got, ref in ((both.input_launch(), plain.input_launch()), (both.out_launch(64, 96), plain.out_launch(64, 96)),
                     (both.deep_launch(64, 96), plain.deep_launch(64, 96))):
        assert got[1] == ref[1]                                     # the argument lists are the planar ones
    only_in = Yuv(*args, depth=10, out_depth=12, layout='semi', out_layout='planar')
    assert [only_in.input_launch()[0], only_in.out_launch(64, 96)[0], only_in.deep_launch(64, 96)[0]] == \
        [NEW[0], PLANAR[1], PLANAR[2]]
    only_out = Yuv(*args, depth=10, out_depth=12, out_layout='semi')
    assert [only_out.input_launch()[0], only_out.out_launch(64, 96)[0], only_out.deep_launch(64, 96)[0]] == \
        [PLANAR[0], NEW[1], NEW[2]]
    old = Yuv420(16, 24)
    assert (old.layout, old.out_layout) == ('planar', None)
    assert old.input_launch()[0] == 'tg_yuv420_to_rgb_f32' and old.out_launch(64, 96)[0] == 'tg_rgb_u8_to_yuv420'


def test_deinterlace_refuses_semi_planar_input():
    from tecogan_pytorch_amd.models.networks import Deinterlace, Yuv
    Deinterlace().check_source(Yuv(16, 24))
    Deinterlace().check_source(Yuv(16, 24, out_layout='semi'))      # (the output's layout is not the deinterlacer's)
    with pytest.raises(ValueError, match='semi-planar'):
        Deinterlace().check_source(Yuv(16, 24, layout='semi'))


def test_raw_reader_and_writer_round_trip_and_the_short_frame_error():
    from tecogan_pytorch_amd.data import rawvideo as RV
    assert RV.FORMATS == S.FORMATS
    assert sorted(RV.FORMATS) == sorted('nv12 nv16 nv24 p010 p012 p210 p212 p410 p412'.split())
    for fmt, (chroma, depth) in RV.FORMATS.items():
        h, w, t = 5, 7, 3
        fb = P.frame_bytes(h, w, chroma, depth)
        assert RV.frame_bytes(h, w, chroma, depth) == fb
        frames = np.random.default_rng(fb).integers(0, 256, (t, fb), dtype=np.uint8)
        f = io.BytesIO()
        wr = RV.RawWriter(f, fb)
        for fr in frames:
            wr.write(fr if depth == 8 else fr.view(np.uint16))
        wr.flush()
        assert f.getvalue() == frames.tobytes()                     # nothing in between
        with pytest.raises(RV.RawVideoError, match=str(fb)):
            wr.write(frames[0][:-1])
        rd = RV.RawReader(io.BytesIO(f.getvalue()), fmt, w, h)
        assert (rd.w, rd.h, rd.chroma, rd.depth, rd.frame_bytes) == (w, h, chroma, depth, fb)
        got = np.stack([fr.copy() for fr in rd])
        assert np.array_equal(got, frames) and rd.frames_read == t
        short = RV.RawReader(io.BytesIO(f.getvalue()[:fb + 5]), fmt, w, h)
        assert np.array_equal(next(short), frames[0])
        with pytest.raises(RV.RawVideoError, match=f'5 of {fb} bytes'):
            next(short)
    assert RV.format_of('P010LE') == ('420', 10) and RV.format_of('NV24') == ('444', 8)
    for bad in ('nv21', 'p016', 'yuyv422', 'nv12le', '', None):
        with pytest.raises(RV.RawVideoError):
            RV.format_of(bad)
    with pytest.raises(RV.RawVideoError):
        RV.RawReader(io.BytesIO(b''), 'nv12', 1, 8)

    class Dribble(io.RawIOBase):                                    # a pipe that hands over 3 bytes at a time, no readinto
        def __init__(self, data):
            self.data, self.at = data, 0

        def read(self, n=-1):
            piece = self.data[self.at:self.at + min(3, n)]
            self.at += len(piece)
            return piece
        readinto = None
    frames = np.arange(2 * 12, dtype=np.uint8).reshape(2, 12)
    assert np.array_equal(np.stack([fr.copy() for fr in RV.RawReader(Dribble(frames.tobytes()), 'nv24', 2, 2)]), frames)


def test_parse_args_refusals(tmp_path, capsys):
    from tecogan_pytorch_amd import main as M
    src = tmp_path / 'in.yuv'
    src.write_bytes(b'\0' * 12)
    base = ['--mode', 'infer', '--input', str(src), '--output', str(tmp_path / 'out.yuv')]
    ok = M.parse_args(base + ['--raw-format', 'p010le', '--raw-size', '320x134'])
    assert (ok.raw_format, ok.raw_size, ok.raw_rate, ok.output_format) == ('p010', (320, 134), None, None)
    ok = M.parse_args(base + ['--raw-format', 'nv12', '--raw-size', '4x2', '--raw-rate', '30000:1001', '--output-format', 'y4m'])
    assert (ok.raw_rate, ok.output_format) == ((30000, 1001), 'y4m')
    assert M.parse_args(base + ['--output-format', 'raw']).output_format == 'raw'       # raw output from y4m input
    for extra, word in ((['--raw-format', 'nv12'], '--raw-size'),
                        (['--raw-format', 'nv12', '--raw-size', '4x2', '--deinterlace', 'tff'], '--deinterlace'),
                        (['--raw-size', '4x2'], '--raw-format'),
                        (['--raw-rate', '25:1'], '--raw-format'),
                        (['--raw-format', 'nv21', '--raw-size', '4x2'], 'nv21'),
                        (['--raw-format', 'nv12', '--raw-size', '4'], 'WxH'),
                        (['--raw-format', 'nv12', '--raw-size', '4x2', '--raw-rate', '25'], 'N:D')):
        with pytest.raises(SystemExit) as e:
            M.parse_args(base + extra)
        assert e.value.code == 2
        assert word in capsys.readouterr().err
    with pytest.raises(SystemExit):                                 # a folder of PNGs has no raw format
        M.parse_args(['--mode', 'infer', '--input', str(tmp_path), '--output', str(tmp_path), '--raw-format', 'nv12',
                      '--raw-size', '4x2'])
    capsys.readouterr()


def test_header_declares_the_three_entry_points_with_the_planar_argument_lists():
    from tecogan_pytorch_amd import _lib as L
    text = open(os.path.join(ROOT, 'include', 'tecogan_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for new, old in zip(NEW, PLANAR):
        assert len(re.findall(r'\b%s\s*\(' % new, text)) == 1
        assert L.SIGNATURES[new] == L.SIGNATURES[old]
    assert L.TG_ABI_MAJOR == 2 and len(L.STRUCTS) == 7
