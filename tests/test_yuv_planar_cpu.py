"""Planar YUV 4:2:0 / 4:2:2 / 4:4:4 at 8, 10 and 12 bits and the BT.2020 matrix, without a GPU:
the numpy specification tests/yuv_planar_ref.py against the pinned tables, against the two 4:2:0 specifications it
generalises, and against the fp64 route; and the plumbing above the kernels -- the Yuv dataclass, yuv_planes, the y4m
reader and writer for the six new headers, the refusals that come before anything is pulled, the CLI's arguments."""
import io
import os
import re

import numpy as np
import pytest
import torch

from tests import yuv_depth_ref as RD
from tests import yuv_planar_ref as P
from tests import yuv_ref as R8
from tests.test_yuv_cpu import TABLES as TABLES_8
from tecogan_pytorch_amd import _lib as L
from tecogan_pytorch_amd.data.y4m import Y4MError, Y4MReader, Y4MWriter, frame_bytes, parse_header
from tecogan_pytorch_amd.models.networks import Yuv, Yuv420, yuv_planes, yuv420_planes
from tecogan_pytorch_amd.models.networks import tecogan_nets as N
from tecogan_pytorch_amd.models.networks.stream import Resize, stream_parts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL3 = ('420', '422', '444')


# ---------------------------------------------------------------- tables
@pytest.mark.parametrize('matrix,full', R8.CONFIGS)
def test_computed_tables_equal_the_pinned_bt601_and_bt709_tables(matrix, full):
    assert P.q_table(8, matrix, full).tolist() == TABLES_8[(matrix, full)]
    for depth in (10, 12):
        assert P.q_table(depth, matrix, full).tolist() == RD.TABLES[(depth, matrix, full)]


def test_bt2020_tables_equal_the_ones_printed_in_the_design_document():
    text = open(os.path.join(ROOT, 'DESIGN.md')).read()
    sec = text[text.index('\n## 7l. '):]
    rows = re.findall(r'^\| (8|10|12) \| (limited|full) \| ([-\d ]+) \| ([-\d ]+) \| ([-\d ]+) \|$', sec, flags=re.M)
    assert len(rows) == 6
    for depth, rng, y, cb, cr in rows:
        printed = [[int(v) for v in row.split()] for row in (y, cb, cr)]
        key = (int(depth), rng == 'full')
        assert printed == P.BT2020_TABLES[key] == P.q_table(key[0], 'bt2020', key[1]).tolist(), key
    assert P.KR_KB['bt2020'] == (0.2627, 0.0593)
    # a row of Y sums to ys / in * 2^sh, the chroma rows to 0, within the roundings
    for (depth, full), t in P.BT2020_TABLES.items():
        _, ys, _, _ = P.scales(depth, full)
        one, top = (65536, 255) if depth == 8 else (1 << 24, 65535)
        assert abs(sum(t[0]) - ys / top * one) <= 1.5 and abs(sum(t[1])) <= 1 and abs(sum(t[2])) <= 1


def test_the_enum_tables_of_the_binding():
    assert L.YUV_PLANAR_MATRIX == {'bt601': 0, 'bt709': 1, 'bt2020': 2} and L.YUV_MATRIX == {'bt601': 0, 'bt709': 1}
    assert L.YUV_CHROMA == {'420': 0, '422': 1, '444': 2}
    for name in ('tg_yuv_planar_to_rgb_f32', 'tg_rgb_u8_to_yuv_planar', 'tg_rgb_f32_to_yuv_planar16'):
        assert name in L.SIGNATURES


# ---------------------------------------------------------------- the specification at 4:2:0 is the two existing ones
def _rgb_u8(n, H, W, seed):
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    x[0, :, : max(1, W // 2)] = rng.choice(np.array([0, 255], np.uint8), (H, max(1, W // 2), 3))     # saturated primaries
    return x


def _rgb_f32(n, H, W, seed):
    rng = np.random.default_rng(seed)
    x = (rng.random((n, 3, H, W), dtype=np.float32) * np.float32(1.5) - np.float32(0.25)).astype(np.float32)
    x[0, :, 0, 0] = np.nan
    return x


@pytest.mark.parametrize('siting', P.SITINGS)
@pytest.mark.parametrize('matrix,full', R8.CONFIGS)
def test_specification_at_420_equals_the_two_existing_specifications_byte_for_byte(matrix, full, siting):
    for H, W in ((2, 2), (4, 6), (6, 8), (10, 14)):
        x = _rgb_u8(2, H, W, H * W)
        assert np.array_equal(P.rgb_u8_to_yuv(x, '420', matrix, full, siting), R8.rgb_to_yuv420(x, matrix, full, siting))
        f = _rgb_f32(2, H, W, H + W)
        for depth in (10, 12):
            assert np.array_equal(P.rgb_f32_to_yuv(f, '420', depth, matrix, full, siting),
                                  RD.rgb_f32_to_yuv420p(f, depth, matrix, full, siting))
    rng = np.random.default_rng(5)
    for h, w in ((2, 2), (3, 5), (9, 11), (8, 12)):
        y8 = rng.integers(0, 256, (2, R8.frame_bytes(h, w)), dtype=np.uint8)
        assert np.array_equal(P.yuv_to_rgb(y8, h, w, '420', 8, matrix, full, siting),
                              R8.yuv420_to_rgb(y8, h, w, matrix, full, siting))
        for depth in (10, 12):
            y16 = rng.integers(0, 65536, (2, RD.frame_samples(h, w)), dtype=np.uint16)
            assert np.array_equal(P.yuv_to_rgb(y16, h, w, '420', depth, matrix, full, siting),
                                  RD.yuv420p_to_rgb(y16, h, w, depth, matrix, full, siting))


# ---------------------------------------------------------------- closeness to fp64, grey
@pytest.mark.parametrize('chroma', P.CHROMAS)
@pytest.mark.parametrize('depth', P.DEPTHS)
def test_integer_output_is_within_one_code_of_the_fp64_route(chroma, depth, capsys):
    """The integer formula rounds Q once per entry: against colours_to_ycc_f64 on the exact tap average, rounded half
    up, it may land on the neighbouring code, never further.  The share of samples that differ at all is reported."""
    rng = np.random.default_rng(depth * 7 + len(chroma))
    H, W = 24, 32
    top_in = 255 if depth == 8 else 65535
    p = rng.integers(0, top_in + 1, (4, H, W, 3)).astype(np.int64)
    p[0, :8] = rng.choice(np.array([0, top_in]), (8, W, 3))           # saturated primaries: the clip
    shares = []
    for siting in P.SITINGS:
        for matrix, full in P.CONFIGS:
            a = P.ints_to_yuv(p, chroma, depth, matrix, full, siting)
            b = P.ints_to_yuv_f64(p, chroma, depth, matrix, full, siting)
            assert a.shape == b.shape == (4, P.frame_samples(H, W, chroma))
            d = np.abs(a - b)
            assert d.max() <= 1, (siting, matrix, full, int(d.max()))
            shares.append(((siting, matrix, full), float((d > 0).mean())))
    with capsys.disabled():
        worst = max(shares, key=lambda s: s[1])
        print('\n4:%s:%s at %d bits: samples off the fp64 route by one code: worst %.4f%% (%s), mean %.4f%%'
              % (chroma[1], chroma[2], depth, 100 * worst[1], worst[0], 100 * np.mean([s[1] for s in shares])))


@pytest.mark.parametrize('chroma', P.CHROMAS)
def test_grey_gives_the_mid_chroma_code_in_every_layout(chroma):
    H, W = 4, 8
    for depth in P.DEPTHS:
        top_in = 255 if depth == 8 else 65535
        levels = np.unique(np.concatenate([np.arange(0, top_in + 1, max(1, top_in // 255)), [top_in]]))
        for siting in P.SITINGS:
            for matrix, full in P.CONFIGS:
                mid = P.scales(depth, full)[3]
                p = np.broadcast_to(levels[:, None, None, None], (levels.size, H, W, 3)).astype(np.int64)
                _, u, v = P.planes(P.ints_to_yuv(p, chroma, depth, matrix, full, siting), H, W, chroma)
                assert (u == mid).all() and (v == mid).all(), (depth, siting, matrix, full)


def test_444_input_sample_is_16_c_and_the_taps_of_every_layout_sum_to_16():
    for chroma in P.CHROMAS:
        for siting in P.SITINGS:
            for h, w in ((2, 2), (3, 5), (9, 11)):
                ch, cw = P.chroma_size(h, w, chroma)
                assert (P.upsample16(np.ones((1, ch, cw), np.int64), h, w, chroma, siting) == 16).all()
    c = np.arange(15, dtype=np.int64).reshape(1, 3, 5)
    assert np.array_equal(P.upsample16(c, 3, 5, '444', 'left'), 16 * c)
    # 4:2:2 has no vertical mixing: every row is its own chroma row
    c = np.arange(9, dtype=np.int64).reshape(1, 3, 3) * 100
    up = P.upsample16(c, 3, 5, '422', 'left')
    assert np.array_equal(up[0, :, 0::2], 16 * c[0]) and np.array_equal(up[0, :, 1], 8 * (c[0, :, 0] + c[0, :, 1]))


# ---------------------------------------------------------------- Yuv
def test_yuv_validation_and_byte_counts():
    y = Yuv(9, 11)
    assert (y.chroma, y.oc, y.matrix, y.full_range, y.siting, y.depth, y.od) == ('420', '420', 'bt709', False, 'left', 8, 8)
    assert y.frame_bytes == Yuv420(9, 11).frame_bytes == 99 + 2 * 5 * 6
    assert Yuv(9, 11, chroma='422').frame_bytes == 99 + 2 * 9 * 6
    assert Yuv(9, 11, chroma='444').frame_bytes == 3 * 99
    assert Yuv(9, 11, chroma='422', depth=10).frame_bytes == 2 * (99 + 2 * 9 * 6)
    assert Yuv(9, 11, chroma='444', depth=12).frame_bytes == 2 * 3 * 99
    for c in ALL3:
        for d in (8, 10, 12):
            assert Yuv(9, 11, chroma=c, depth=d).frame_bytes == P.frame_bytes(9, 11, c, d) == frame_bytes(9, 11, d, c)
    H, W = 36, 44
    assert Yuv(9, 11).out_frame_bytes(4) == H * W * 3 // 2 == Yuv420(9, 11).out_frame_bytes(4)
    assert Yuv(9, 11, out_chroma='422').out_frame_bytes(4) == 2 * H * W
    assert Yuv(9, 11, chroma='444', out_chroma='420').out_frame_bytes(4) == H * W * 3 // 2
    assert Yuv(9, 11, out_chroma='444', out_depth=12).out_frame_bytes(4) == 2 * 3 * H * W
    assert Yuv(9, 11, chroma='422', depth=10).out_frame_bytes(2) == 2 * 2 * 18 * 22
    y = Yuv(9, 11, chroma='422', out_chroma='444', matrix='bt2020', full_range=True, siting='center', depth=10, out_depth=8)
    assert (y.oc, y.od) == ('444', 8) and y.codes() == (2, 1, 0)
    assert Yuv(8, 8, matrix='bt601').codes() == (0, 0, 1)
    assert Yuv(9, 11, out_chroma='422').out_size_bytes(5, 6) == 5 * 6 * 2
    assert Yuv(9, 11, out_chroma='444').out_size_bytes(5, 7) == 5 * 7 * 3
    with pytest.raises(ValueError, match='even width'):
        Yuv(9, 11, out_chroma='422').out_size_bytes(6, 7)
    with pytest.raises(ValueError, match='even sides'):
        Yuv(9, 11).out_size_bytes(5, 6)
    with pytest.raises(Exception):
        y.h = 3                                      # frozen
    for bad in (dict(chroma='411'), dict(chroma=420), dict(out_chroma='400'), dict(matrix='bt2100'), dict(matrix=2),
                dict(siting='top'), dict(full_range=1), dict(depth=9), dict(out_depth=16), dict(depth=True)):
        with pytest.raises(ValueError, match='Yuv:'):
            Yuv(8, 8, **bad)
    for bad in ((1, 8), (8, 1), (8.0, 8), (True, 8)):
        with pytest.raises(ValueError, match='Yuv:'):
            Yuv(*bad)
    with pytest.raises(ValueError, match='Yuv420'):
        Yuv420(8, 8, matrix='bt2020')                # the 4:2:0 class keeps its two matrices


def test_yuv_planes_are_views_of_every_layout():
    H, W = 5, 7
    for chroma in ALL3:
        ch, cw = P.chroma_size(H, W, chroma)
        ns = P.frame_samples(H, W, chroma)
        chunk = np.arange(3 * ns, dtype=np.uint8).reshape(3, ns)
        y, u, v = yuv_planes(chunk, H, W, chroma)
        assert y.shape == (3, H, W) and u.shape == v.shape == (3, ch, cw)
        assert y.base is not None and np.shares_memory(y, chunk) and np.shares_memory(v, chunk)
        ry, ru, rv = P.planes(chunk, H, W, chroma)
        assert np.array_equal(y, ry) and np.array_equal(u, ru) and np.array_equal(v, rv)
        y1, u1, v1 = yuv_planes(torch.from_numpy(chunk[0]), H, W, chroma)
        assert y1.shape == (H, W) and u1.shape == (ch, cw) and torch.equal(v1, torch.from_numpy(rv[0]))
        deep = (np.arange(2 * ns, dtype=np.uint16) * 3).reshape(2, ns)
        for c16 in (deep, deep.view(np.uint8)):
            y, u, v = yuv_planes(c16, H, W, chroma, depth=10)
            assert y.dtype == np.uint16 and np.array_equal(v, P.planes(deep, H, W, chroma)[2])
        with pytest.raises(ValueError, match='yuv_planes'):
            yuv_planes(chunk[:, :-1], H, W, chroma)
    a, b = yuv_planes(np.zeros(Yuv420(5, 7).frame_bytes, np.uint8), 5, 7), yuv420_planes(np.zeros(Yuv420(5, 7).frame_bytes, np.uint8), 5, 7)
    assert [p.shape for p in a] == [p.shape for p in b]
    with pytest.raises(ValueError, match='chroma'):
        yuv_planes(np.zeros(10, np.uint8), 2, 2, '411')
    with pytest.raises(ValueError, match='depth'):
        yuv_planes(np.zeros(12, np.uint8), 2, 2, '444', depth=9)


def test_stream_parts_checks_items_against_a_yuv():
    spec = Yuv(5, 7, chroma='422', depth=10)
    fb = spec.frame_bytes
    assert fb == 2 * (35 + 2 * 5 * 4)
    parts = list(stream_parts([np.zeros(fb, np.uint8), np.zeros((2, fb // 2), np.uint16)], 3, spec))
    assert [(k, tuple(x.shape)) for k, x in parts] == [('yuv', (1, fb)), ('yuv', (2, fb))]
    with pytest.raises(ValueError):
        list(stream_parts([np.zeros(Yuv(5, 7, depth=10).frame_bytes, np.uint8)], 3, spec))      # a 4:2:0 frame


def test_refusals_come_before_anything_is_pulled():
    net = N.FRNet(3, 3, 64, 10, 'BD', 4)
    pulled = []

    def items():
        pulled.append(1)
        yield np.zeros(Yuv(8, 8).frame_bytes, np.uint8)
    with pytest.raises(ValueError, match='8-bit'):
        net.infer_stream(items(), device='cpu', yuv=Yuv(8, 8, out_chroma='444', out_depth=10), resize=Resize(16, 16))
    with pytest.raises(ValueError, match='even width'):
        net.infer_stream(items(), device='cpu', yuv=Yuv(8, 8, out_chroma='422'), resize=Resize(16, 17))
    with pytest.raises(ValueError, match='even sides'):
        net.infer_stream(items(), device='cpu', yuv=Yuv(8, 8, chroma='444', out_chroma='420'), resize=Resize(17, 16))
    with pytest.raises(ValueError, match='I420'):
        net.infer_stream(items(), device='cpu', yuv=Yuv420(8, 8), resize=Resize(17, 16))       # (the 4:2:0 class's own)
    with pytest.raises(ValueError, match='png and yuv'):
        net.infer_stream(items(), device='cpu', yuv=Yuv(8, 8), png=N.Png())
    with pytest.raises(ValueError, match='Yuv420, a Yuv or None'):
        net.infer_stream(items(), device='cpu', yuv='444')
    assert pulled == []
    # 4:2:2 takes an odd height, 4:4:4 any size: accepted, and an empty stream ends at once
    for spec, rs in ((Yuv(8, 8, out_chroma='422'), Resize(17, 16)), (Yuv(8, 8, out_chroma='444'), Resize(17, 15))):
        assert list(net.infer_stream(iter([]), device='cpu', yuv=spec, resize=rs)) == []


# ---------------------------------------------------------------- y4m
NEW_TAGS = [('422', '422', 8), ('444', '444', 8), ('422p10', '422', 10), ('422p12', '422', 12), ('444p10', '444', 10),
            ('444p12', '444', 12)]


def _y4m(header, frames):
    return io.BytesIO(header + b'\n' + b''.join(b'FRAME\n' + f.tobytes() for f in frames))


@pytest.mark.parametrize('tag', ['422', '444', '444p10', '422p12'])
def test_default_reader_still_refuses_the_new_headers_by_name(tag):
    for mk in (lambda: parse_header(b'YUV4MPEG2 W4 H4 C' + tag.encode()),
               lambda: Y4MReader(io.BytesIO(b'YUV4MPEG2 W4 H4 C' + tag.encode() + b'\n'))):
        with pytest.raises(Y4MError) as e:
            mk()
        assert f'C{tag}' in str(e.value) and str(e.value).endswith('(supported: C420jpeg, C420mpeg2, C420)')
    if 'p1' in tag:                                   # ... and a reader opened for all depths, as before this layout existed
        with pytest.raises(Y4MError) as e:
            parse_header(b'YUV4MPEG2 W4 H4 C' + tag.encode(), (8, 10, 12))
        assert str(e.value).endswith('(supported: C420jpeg, C420mpeg2, C420, C420p10, C420p12)')


@pytest.mark.parametrize('tag,chroma,depth', NEW_TAGS)
def test_reader_opened_for_all_layouts_reads_the_six_new_headers(tag, chroma, depth):
    h, w = 5, 7
    fb = P.frame_bytes(h, w, chroma, depth)
    rng = np.random.default_rng(depth)
    frames = [rng.integers(0, 256, fb, dtype=np.uint8) for _ in range(3)]
    head = b'YUV4MPEG2 W7 H5 F30:1 Ip A1:1 C' + tag.encode() + b' XCOLORRANGE=FULL'
    rd = Y4MReader(_y4m(head, frames), depths=(8, 10, 12), chromas=ALL3)
    assert (rd.w, rd.h, rd.chroma, rd.depth, rd.siting, rd.full_range, rd.frame_bytes) == (7, 5, chroma, depth, None, True, fb)
    assert rd.header['chroma'] == chroma and 'C' + tag in rd.header['tags']
    got = [f.copy() for f in rd]
    assert len(got) == 3 and all(np.array_equal(a, b) for a, b in zip(got, frames))

    class Dribble(io.RawIOBase):                      # short reads: a pipe that hands out 3 bytes at a time
        def __init__(self, data):
            self.b = io.BytesIO(data)

        def readable(self):
            return True

        def readinto(self, view):
            piece = self.b.read(min(3, len(view)))
            view[:len(piece)] = piece
            return len(piece)
    rd = Y4MReader(io.BufferedReader(Dribble(_y4m(head, frames).getvalue()), buffer_size=16), depths=(8, 10, 12), chromas=ALL3)
    assert all(np.array_equal(a.copy(), b) for a, b in zip(rd, frames)) and rd.frames_read == 3
    cut = _y4m(head, frames).getvalue()[:-5]
    rd = Y4MReader(io.BytesIO(cut), depths=(8, 10, 12), chromas=ALL3)
    next(rd), next(rd)
    with pytest.raises(Y4MError, match='ends inside frame 2'):
        next(rd)
    if depth > 8:                                     # the depth must be allowed as well
        with pytest.raises(Y4MError, match='C' + tag):
            Y4MReader(_y4m(head, frames), chromas=ALL3)


def test_reader_opened_for_all_layouts_takes_420_as_before_and_refuses_the_rest_by_name():
    for head, siting, depth in ((b'C420jpeg', 'center', 8), (b'C420mpeg2', 'left', 8), (b'C420', 'center', 8), (b'', 'center', 8),
                                (b'C420p10', None, 10)):
        hd = parse_header(b'YUV4MPEG2 W4 H4 ' + head, (8, 10, 12), ALL3)
        assert (hd['chroma'], hd['siting'], hd['depth']) == ('420', siting, depth)
        assert parse_header(b'YUV4MPEG2 W4 H4 ' + head, (8, 10, 12))['chroma'] == '420'
    for tag in ('mono', 'mono12', '411', '444alpha', '420p14', '422p16', '444p14', '420paldv', '440'):
        with pytest.raises(Y4MError) as e:
            parse_header(b'YUV4MPEG2 W4 H4 C' + tag.encode(), (8, 10, 12), ALL3)
        assert f'C{tag}:' in str(e.value) and 'C444p12' in str(e.value)
    with pytest.raises(Y4MError, match='interlaced'):
        parse_header(b'YUV4MPEG2 W4 H4 It C422', (8,), ALL3)
    with pytest.raises(Y4MError, match='C444'):
        parse_header(b'YUV4MPEG2 W4 H4 C444', (8,), ('420', '422'))


@pytest.mark.parametrize('tag,chroma,depth', NEW_TAGS)
def test_writer_reader_round_trip_and_tags(tag, chroma, depth):
    H, W = 6, 10
    src = parse_header(b'YUV4MPEG2 W5 H3 F25:1 Ip A1:1 C420mpeg2 XYSCSS=420MPEG2 XCOLORRANGE=LIMITED')
    out = io.BytesIO()
    wr = Y4MWriter(out, W, H, src, depth=depth, chroma=chroma)
    assert wr.frame_bytes == P.frame_bytes(H, W, chroma, depth)
    frames = [np.full(wr.frame_bytes, k, np.uint8) for k in range(2)]
    for f in frames:
        wr.write(f)
    with pytest.raises(Y4MError):
        wr.write(frames[0][:-1])
    line = out.getvalue().split(b'\n', 1)[0].decode()
    assert line == f'YUV4MPEG2 W10 H6 F25:1 A1:1 C{tag} XYSCSS={tag.upper()} XCOLORRANGE=LIMITED Ip'
    rd = Y4MReader(io.BytesIO(out.getvalue()), depths=(8, 10, 12), chromas=ALL3)
    assert (rd.chroma, rd.depth, rd.full_range) == (chroma, depth, False)
    assert all(np.array_equal(a.copy(), b) for a, b in zip(rd, frames))
    # without a header to take tags from, and after an input that had no XYSCSS: the twin is written all the same
    bare = io.BytesIO()
    Y4MWriter(bare, W, H, None, depth=depth, chroma=chroma)
    assert bare.getvalue().decode() == f'YUV4MPEG2 W10 H6 C{tag} XYSCSS={tag.upper()} Ip\n'


def test_writer_420_after_another_layout_and_the_unchanged_defaults():
    src = parse_header(b'YUV4MPEG2 W4 H4 F25:1 C444 XYSCSS=444', (8,), ALL3)
    out = io.BytesIO()
    Y4MWriter(out, 8, 8, src, siting='center', chroma='420')
    assert out.getvalue() == b'YUV4MPEG2 W8 H8 F25:1 C420jpeg XYSCSS=420JPEG Ip\n'
    with pytest.raises(Y4MError, match='siting'):
        Y4MWriter(io.BytesIO(), 8, 8, src)
    with pytest.raises(Y4MError, match='chroma'):
        Y4MWriter(io.BytesIO(), 8, 8, None, chroma='411')
    # a 4:2:0 writer writes what it wrote: chroma=None and '420' are the same header
    src = parse_header(b'YUV4MPEG2 W4 H4 F25:1 C420mpeg2')
    a, b = io.BytesIO(), io.BytesIO()
    Y4MWriter(a, 8, 8, src)
    Y4MWriter(b, 8, 8, src, chroma='420')
    assert a.getvalue() == b.getvalue() == b'YUV4MPEG2 W8 H8 F25:1 C420mpeg2 Ip\n'


# ---------------------------------------------------------------- the CLI's arguments
def test_cli_output_chroma_and_matrix_arguments(tmp_path):
    from tecogan_pytorch_amd import main as M
    y4m = tmp_path / 'clip.y4m'
    y4m.write_bytes(b'YUV4MPEG2 W4 H2 C422p10\n')
    folder = str(tmp_path)
    a = M.parse_args(['--mode', 'infer', '--input', str(y4m), '--output', '-'])
    assert (a.output_chroma, a.yuv_matrix) == (None, 'bt709')
    a = M.parse_args(['--mode', 'infer', '--input', '-', '--output', '-', '--output-chroma', '444', '--yuv-matrix', 'bt2020'])
    assert (a.output_chroma, a.yuv_matrix) == ('444', 'bt2020')
    assert M.parse_args(['--mode', 'infer', '--input', str(y4m), '--output-chroma', '422', '--output-depth', '12']).output_chroma == '422'
    for bad in (['--mode', 'infer', '--input', folder, '--output-chroma', '444'],          # a PNG folder
                ['--mode', 'infer', '--output-chroma', '444'],                             # no input at all
                ['--mode', 'test', '--input', str(y4m), '--output-chroma', '444'],
                ['--mode', 'infer', '--input', str(y4m), '--output-chroma', '411'],
                ['--mode', 'infer', '--input', str(y4m), '--output-chroma', '4:4:4'],
                ['--mode', 'infer', '--input', str(y4m), '--yuv-matrix', 'bt2100']):
        with pytest.raises(SystemExit) as e:
            M.parse_args(bad)
        assert e.value.code == 2, bad
