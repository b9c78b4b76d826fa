"""Host side of the raw-video path (no GPU): the integer tables and how close the integer output
formula is to fp64 over ALL 2^24 colours, the round trip, the chroma up-sampling taps, the y4m reader / writer, Yuv420,
and the front padding of I420 streams."""
import io
import os
import threading

import numpy as np
import pytest
import torch

from tests import yuv_ref as R
from tecogan_pytorch_amd.data.y4m import Y4MError, Y4MReader, Y4MWriter
from tecogan_pytorch_amd.models.base_model import BaseModel, front_pad_stream
from tecogan_pytorch_amd.models.networks import Yuv420, yuv420_planes
from tecogan_pytorch_amd.models.networks import tecogan_nets as N

TABLES = {
    ('bt601', False): [[16829, 33039, 6416], [-9714, -19071, 28784], [28784, -24103, -4681]],
    ('bt601', True): [[19595, 38470, 7471], [-11058, -21710, 32768], [32768, -27439, -5329]],
    ('bt709', False): [[11966, 40254, 4064], [-6596, -22189, 28784], [28784, -26145, -2639]],
    ('bt709', True): [[13933, 46871, 4732], [-7509, -25259, 32768], [32768, -29763, -3005]],
}


@pytest.mark.parametrize('matrix,full', R.CONFIGS)
def test_q_tables_follow_from_kr_and_kb(matrix, full):
    assert R.q_table(matrix, full).tolist() == TABLES[(matrix, full)]


def _colour_slabs():
    """All 2^24 colours, one value of R at a time: (65536, 3) int64."""
    g, b = np.meshgrid(np.arange(256), np.arange(256), indexing='ij')
    gb = np.stack([g.ravel(), b.ravel()], 1)
    for r in range(256):
        yield np.concatenate([np.full((65536, 1), r), gb], 1).astype(np.int64)


@pytest.mark.parametrize('matrix,full', R.CONFIGS)
def test_integer_formula_against_fp64_over_all_colours(matrix, full):
    """Both sides clipped to [0, 255], the output's range (full-range chroma of pure blue / red is 255.5 -> 256)."""
    differing, worst = np.zeros(3, np.int64), 0
    for rgb in _colour_slabs():
        got = R.colours_to_ycc_int(rgb, matrix, full)
        ref = np.clip(np.floor(R.colours_to_ycc_f64(rgb, matrix, full) + 0.5), 0, 255).astype(np.int64)
        d = np.abs(got - ref)
        worst = max(worst, int(d.max()))
        differing += (d != 0).sum(0)
    share = differing / float(1 << 24)
    print(matrix, 'full' if full else 'limited', 'differing share per plane', share, 'worst', worst)
    assert worst <= 1
    assert (share <= 0.0025).all(), share


@pytest.mark.parametrize('matrix,full', R.CONFIGS)
def test_constant_colour_round_trip_over_all_colours(matrix, full):
    worst = 0.0
    for rgb in _colour_slabs():
        ycc = R.colours_to_ycc_int(rgb, matrix, full)
        back = R.ycc_to_rgb_f64(ycc[:, 0], ycc[:, 1] * 16, ycc[:, 2] * 16, matrix, full) * 255.0     # (3, 65536)
        worst = max(worst, float(np.abs(back.T - rgb).max()))
    print(matrix, 'full' if full else 'limited', 'round trip worst', worst)
    assert worst <= 2.0


@pytest.mark.parametrize('h,w', [(2, 2), (3, 3), (8, 8), (9, 11), (13, 34), (16, 258)])
@pytest.mark.parametrize('siting', R.SITINGS)
def test_upsampling_weights_sum_to_16_everywhere(h, w, siting):
    ch, cw = (h + 1) // 2, (w + 1) // 2
    ri, rw = R.upsample_taps(h, ch, 'center')
    ci, cwt = R.upsample_taps(w, cw, siting)
    assert ri.min() >= 0 and ri.max() <= ch - 1 and ci.min() >= 0 and ci.max() <= cw - 1
    total = np.zeros((h, w, ch, cw), np.int64)                  # the weight of every chroma sample in every pixel
    for a in range(2):
        for b in range(2):
            np.add.at(total, (np.arange(h)[:, None], np.arange(w)[None, :], ri[:, a][:, None], ci[:, b][None, :]),
                      rw[:, a][:, None] * cwt[:, b][None, :])
    assert (total >= 0).all() and (total.sum((2, 3)) == 16).all()
    # a constant plane comes back as the constant, in sixteenths, corners and odd edges included
    assert (R.upsample16(np.full((1, ch, cw), 77), h, w, siting) == 16 * 77).all()


# ---------------------------------------------------------------- y4m
def _clip(n, h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (n, R.frame_bytes(h, w)), dtype=np.uint8)


def _y4m(header, frames, frame_line=b'FRAME\n'):
    return header + b''.join(frame_line + f.tobytes() for f in frames)


def test_y4m_header_round_trip():
    frames = _clip(3, 6, 10)
    src = _y4m(b'YUV4MPEG2 W10 H6 F30000:1001 Ip A1:1 C420mpeg2 XYSCSS=420MPEG2 XCOLORRANGE=FULL\n', frames)
    rd = Y4MReader(io.BytesIO(src))
    assert (rd.w, rd.h, rd.siting, rd.full_range, rd.frame_bytes) == (10, 6, 'left', True, 90)
    assert rd.header['tags'] == ['F30000:1001', 'A1:1', 'C420mpeg2', 'XYSCSS=420MPEG2', 'XCOLORRANGE=FULL']
    got = [f.copy() for f in rd]
    assert len(got) == 3 and all(np.array_equal(g, f) for g, f in zip(got, frames))
    out = io.BytesIO()
    wr = Y4MWriter(out, 40, 24, rd.header)
    big = _clip(2, 24, 40, seed=1)
    for f in big:
        wr.write(f)
    wr.flush()
    head = out.getvalue().split(b'\n', 1)[0]
    assert head == b'YUV4MPEG2 W40 H24 F30000:1001 A1:1 C420mpeg2 XYSCSS=420MPEG2 XCOLORRANGE=FULL Ip'
    back = Y4MReader(io.BytesIO(out.getvalue()))
    assert (back.w, back.h, back.siting, back.full_range) == (40, 24, 'left', True)
    assert back.header['tags'] == rd.header['tags']
    assert all(np.array_equal(g, f) for g, f in zip([f.copy() for f in back], big)) and back.frames_read == 2
    with pytest.raises(Y4MError, match='bytes'):
        wr.write(big[0][:-1])


@pytest.mark.parametrize('head,siting,full', [(b'YUV4MPEG2 W4 H2', 'center', None), (b'YUV4MPEG2 W4 H2 C420', 'center', None),
                                              (b'YUV4MPEG2 W4 H2 C420jpeg XCOLORRANGE=LIMITED', 'center', False),
                                              (b'YUV4MPEG2 W4 H2 F25:1 C420mpeg2', 'left', None)])
def test_y4m_accepted_headers(head, siting, full):
    rd = Y4MReader(io.BytesIO(head + b'\n'))
    assert (rd.siting, rd.full_range) == (siting, full) and list(rd) == []


@pytest.mark.parametrize('tag', ['C420paldv', 'C422', 'C444', 'Cmono', 'C420p10', 'C420p12', 'C420p16', 'C444p10',
                                 'It', 'Ib', 'Im'])
def test_y4m_refusals_name_the_tag(tag):
    with pytest.raises(Y4MError, match=tag):
        Y4MReader(io.BytesIO(b'YUV4MPEG2 W4 H2 F25:1 ' + tag.encode() + b'\n'))


def test_y4m_rejects_what_is_not_y4m():
    with pytest.raises(Y4MError):
        Y4MReader(io.BytesIO(b''))
    with pytest.raises(Y4MError, match='YUV4MPEG2'):
        Y4MReader(io.BytesIO(b'RIFF W4 H2\n'))
    with pytest.raises(Y4MError, match='W and H'):
        Y4MReader(io.BytesIO(b'YUV4MPEG2 W4\n'))
    rd = Y4MReader(io.BytesIO(_y4m(b'YUV4MPEG2 W4 H2\n', _clip(1, 2, 4)) + b'FRAMES\n'))
    next(rd)
    with pytest.raises(Y4MError, match='FRAME line'):
        next(rd)


def test_y4m_frame_line_with_parameters():
    frames = _clip(2, 4, 4)
    rd = Y4MReader(io.BytesIO(_y4m(b'YUV4MPEG2 W4 H4 C420jpeg\n', frames, b'FRAME Ip Xsomething\n')))
    assert all(np.array_equal(g, f) for g, f in zip([f.copy() for f in rd], frames)) and rd.frames_read == 2


@pytest.mark.parametrize('piece', [1, 7, 4099])
def test_y4m_reader_on_a_pipe_written_in_pieces(piece):
    frames = _clip(5, 18, 18, seed=piece)                        # 486 bytes per frame
    data = _y4m(b'YUV4MPEG2 W18 H18 F25:1 C420jpeg\n', frames)
    r, w = os.pipe()

    def feed():
        with os.fdopen(w, 'wb', buffering=0) as f:
            for i in range(0, len(data), piece):
                f.write(data[i:i + piece])
    th = threading.Thread(target=feed)
    th.start()
    try:
        with os.fdopen(r, 'rb', buffering=0) as f:                  # raw: every read may come back short
            got = [x.copy() for x in Y4MReader(f)]
    finally:
        th.join()
    assert len(got) == 5 and all(np.array_equal(g, f) for g, f in zip(got, frames))


def test_y4m_truncated_last_frame_raises():
    frames = _clip(2, 4, 6)
    data = _y4m(b'YUV4MPEG2 W6 H4\n', frames)
    rd = Y4MReader(io.BytesIO(data[:-5]))
    assert np.array_equal(next(rd), frames[0])
    with pytest.raises(Y4MError, match='ends inside frame 1'):
        next(rd)


# ---------------------------------------------------------------- Yuv420 and the stream's host logic
def test_yuv420_validation():
    spec = Yuv420(9, 11)
    assert (spec.matrix, spec.full_range, spec.siting) == ('bt709', False, 'left')
    assert spec.frame_bytes == 99 + 2 * 5 * 6 and spec.out_frame_bytes(2) == 18 * 22 * 3 // 2
    assert spec.out_frame_bytes(4) == 36 * 44 * 3 // 2 and Yuv420(18, 18).frame_bytes == 324 + 2 * 81
    assert spec.codes() == (1, 0, 1) and Yuv420(4, 4, 'bt601', True, 'center').codes() == (0, 1, 0)
    assert spec == Yuv420(9, 11) and spec != Yuv420(9, 11, siting='center') and hash(spec) == hash(Yuv420(9, 11))
    with pytest.raises(AttributeError):
        spec.h = 10
    with pytest.raises(ValueError):
        spec.out_frame_bytes(1)                                  # 9 x 11: odd sides cannot be written as 4:2:0 here
    for bad in (dict(h=1, w=8), dict(h=8, w=0), dict(h=8.0, w=8), dict(h=8, w=8, matrix='bt2020'),
                dict(h=8, w=8, siting='topleft'), dict(h=8, w=8, full_range='full'), dict(h=8, w=8, full_range=1)):
        with pytest.raises(ValueError):
            Yuv420(**bad)
    net = N.FRNet(3, 3, 64, 10, 'BD', 4)
    with pytest.raises(ValueError, match='Yuv420'):
        net.infer_stream(iter([]), device='cpu', yuv=(9, 11))
    assert list(net.infer_stream(iter([]), device='cpu', yuv=spec)) == []


def test_yuv420_planes_are_views():
    chunk = _clip(3, 6, 10)
    y, u, v = yuv420_planes(chunk, 6, 10)
    assert y.shape == (3, 6, 10) and u.shape == v.shape == (3, 3, 5)
    assert all(np.shares_memory(p, chunk) for p in (y, u, v))
    assert np.array_equal(np.concatenate([p.reshape(3, -1) for p in (y, u, v)], 1), chunk)
    y1, u1, v1 = yuv420_planes(torch.from_numpy(chunk[0]), 6, 10)
    assert y1.shape == (6, 10) and u1.shape == (3, 5) and torch.equal(v1, torch.from_numpy(v[0]))
    with pytest.raises(ValueError):
        yuv420_planes(chunk, 6, 12)


def test_stream_parts_refuses_bad_i420_items_before_taking_them():
    spec = Yuv420(6, 10)
    fb = spec.frame_bytes
    ok = [np.zeros(fb, np.uint8), torch.zeros(2, fb, dtype=torch.uint8), np.zeros((0, fb), np.uint8)]
    assert [(k, tuple(x.shape)) for k, x in N.stream_parts(iter(ok), 3, spec)] == [('yuv', (1, fb)), ('yuv', (2, fb))]
    for bad in (np.zeros(fb, np.float32), np.zeros(fb - 1, np.uint8), np.zeros((2, fb + 1), np.uint8),
                np.zeros((6, 10, 3), np.uint8), torch.zeros(fb, dtype=torch.int8), [0] * fb):
        taken = 0
        with pytest.raises(ValueError, match='infer_stream'):
            for _, x in N.stream_parts(iter(ok + [bad]), 3, spec):
                taken += x.shape[0]
        assert taken == 3


class _Pad(BaseModel):
    def __init__(self, mode, n_pad):
        self.opt = {'test': {'padding_mode': mode, 'num_pad_front': n_pad}}


def _pad_sequence_reference(clip, mode, n_pad):
    """BaseModel.pad_sequence (written for 4 axes) on the (t, frame_bytes) clip seen as (t, frame_bytes, 1, 1)."""
    ref, n = _Pad(mode, n_pad).pad_sequence(clip.view(clip.shape[0], -1, 1, 1))
    assert n == n_pad
    return ref.reshape(ref.shape[0], -1)


@pytest.mark.parametrize('mode', ['reflect', 'replicate'])
def test_front_pad_stream_on_i420_items(mode):
    spec = Yuv420(6, 10)
    clip = torch.from_numpy(_clip(11, 6, 10, seed=3))
    for n_pad in (0, 2, 5):
        ref = _pad_sequence_reference(clip, mode, n_pad)
        for items in ([f for f in clip], [f.numpy() for f in clip], [clip[:1], clip[1:4], clip[4:5], clip[5:]],
                      [clip[0], clip[1:9], clip[9], clip[10]]):
            got = torch.cat(list(front_pad_stream(iter(items), mode, n_pad, 3, spec)), 0)
            assert got.shape == ref.shape and torch.equal(got, ref), (n_pad, len(items))
    with pytest.raises(ValueError, match='at least 6'):
        list(front_pad_stream(iter([clip[:5]]), mode, 5, 3, spec))
