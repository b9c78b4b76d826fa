"""The deinterlacer without a GPU: the properties of the numpy specification
(tests/deinterlace_ref.py), the engine's batch-to-window mapping against the specification run once over the whole clip,
the Deinterlace option, the refusals of infer_stream that need no device, the y4m reader and writer, and the flags."""
import io
from types import SimpleNamespace

import numpy as np
import pytest

from tests import deinterlace_ref as R

LAYOUTS = ('420', '422', '444')


def noise(t, h, w, chroma, depth=8, seed=0):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 1 << depth, (t, R.frame_samples(h, w, chroma))).astype(np.uint8 if depth == 8 else np.uint16)


def weave(prog, h, w, chroma, tff):
    """Interlaced frames from 2 t progressive ones: frame i takes the earlier field's rows from picture 2 i and the
    later field's from picture 2 i + 1."""
    out = np.empty((prog.shape[0] // 2, prog.shape[1]), prog.dtype)
    for i in range(out.shape[0]):
        planes = []
        for a, b in zip(R.split(prog[2 * i], h, w, chroma), R.split(prog[2 * i + 1], h, w, chroma)):
            p = a.copy()
            later = 1 if tff else 0                         # the parity of the rows the later field owns
            p[later::2] = b[later::2]
            planes.append(p.reshape(-1))
        out[i] = np.concatenate(planes)
    return out


# ------------------------------------------------------------------ the specification
@pytest.mark.parametrize('tff', [True, False])
@pytest.mark.parametrize('chroma', LAYOUTS)
def test_a_static_scene_is_the_picture_from_frame_1_on(chroma, tff):
    h, w = 8, 10
    pic = noise(1, h, w, chroma, seed=3)
    clip = np.repeat(pic, 4, 0)
    out = R.stream(clip, h, w, chroma, 8, tff)
    assert out.shape[0] == 8 and all(np.array_equal(o, pic[0]) for o in out[2:])
    assert not np.array_equal(out[0], pic[0])               # frame 0 has no frame before: spatial only
    one = R.stream(clip, h, w, chroma, 8, tff, rate='frame')
    assert np.array_equal(one, out[::2])


@pytest.mark.parametrize('tff', [True, False])
@pytest.mark.parametrize('chroma', LAYOUTS)
def test_owned_rows_are_copied_and_frame_0_is_spatial_only(chroma, tff):
    h, w = 8, 12
    clip = noise(3, h, w, chroma, seed=4)
    out = R.stream(clip, h, w, chroma, 8, tff)
    for i, o in enumerate(out):
        t, p = divmod(i, 2)
        par = p ^ (0 if tff else 1)
        for src, dst in zip(R.split(clip[t], h, w, chroma), R.split(o, h, w, chroma)):
            assert np.array_equal(dst[par::2], src[par::2])
    # frame 0's two outputs do not depend on anything but frame 0, and differ from the weave on a moving pair
    alone = R.stream(clip[:1], h, w, chroma, 8, tff)
    assert np.array_equal(alone, out[:2]) and not np.array_equal(out[0], clip[0]) and not np.array_equal(out[1], clip[0])
    # with a frame before, the same two fields come out differently
    warm = R.deinterlace(clip[1:2], h, w, chroma, 8, tff, prev=clip[0])
    assert np.array_equal(warm, out[2:4]) and not np.array_equal(warm, R.stream(clip[1:2], h, w, chroma, 8, tff))


def test_every_output_lies_between_its_three_candidates():
    h, w = 8, 16
    cur, prev = (noise(1, h, w, '444', seed=s)[0][:h * w].reshape(h, w) for s in (5, 6))
    for par in (0, 1):
        for later in (False, True):
            parts, stats = [], {}
            out = R.field_plane(cur, prev, par, later, stats, parts)
            assert len(parts) == h // 2
            for r, sp, tp, m in parts:
                lo = np.minimum(np.minimum(sp, tp - m), tp + m)
                hi = np.maximum(np.maximum(sp, tp - m), tp + m)
                assert (out[r] >= lo).all() and (out[r] <= hi).all()
                assert np.array_equal(out[r], np.minimum(np.maximum(sp, tp - m), tp + m))
            # on unrelated pictures most missing samples are the spatial candidate (about 70 %)
            assert 0.5 < stats['sp'] / stats['n'] < 0.9
            assert all(stats['dir', d] > 0 for d in R.DIRECTIONS) and stats['lo'] > 0 and stats['hi'] > 0


def test_the_direction_rule_ties_go_to_0_then_minus_1():
    a = np.array([10, 10, 10, 10, 10, 10], np.int64)
    assert np.array_equal(R.spatial_row(a, a), a)           # all scores 0: d = 0
    # a diagonal edge: the line through a[x-1], b[x+1] is flat, the vertical pair is not
    a = np.array([0, 0, 0, 100, 100, 100, 100, 100], np.int64)
    b = np.array([0, 0, 0, 0, 0, 100, 100, 100], np.int64)
    stats = {}
    sp = R.spatial_row(a, b, stats)
    assert stats['dir', -1] > 0 and sp[4] == 100 and sp[3] == 0       # d = -1 at x = 4: (a[3] + b[5] + 1) >> 1
    assert (R.spatial_row(b, a)[3:5] == np.array([0, 100])).all()     # mirrored: d = +1


@pytest.mark.parametrize('depth', [10, 12])
def test_a_word_above_the_depths_maximum_acts_as_the_maximum(depth):
    h, w, top = 8, 10, (1 << depth) - 1
    clip = noise(3, h, w, '422', depth, seed=7)
    over = clip.copy()
    clip[:, ::5] = top
    over[:, ::5] = np.array([top + 1, 40000, 65535, top + 7], np.uint16)[np.arange(over[:, ::5].shape[1]) % 4]
    for tff in (True, False):
        a, b = R.stream(clip, h, w, '422', depth, tff), R.stream(over, h, w, '422', depth, tff)
        assert np.array_equal(a, b) and int(b.max()) <= top


@pytest.mark.parametrize('chroma', LAYOUTS)
def test_swapping_the_field_order_on_a_picture_moved_by_one_row_gives_the_moved_result(chroma):
    """A vertically periodic picture (period h) rolled by one row exchanges the row parities; with the other field order
    the fields hold the same samples, so the interior rows of the result are the rolled ones."""
    h, w = 16, 10
    clip = noise(3, h, w, chroma, seed=8)
    rolled = np.stack([np.concatenate([np.roll(p, 1, 0).reshape(-1) for p in R.split(f, h, w, chroma)]) for f in clip])
    a, b = R.stream(clip, h, w, chroma, 8, True), R.stream(rolled, h, w, chroma, 8, False)
    for fa, fb in zip(a, b):
        for pa, pb in zip(R.split(fa, h, w, chroma), R.split(fb, h, w, chroma)):
            assert np.array_equal(pa[1:-2], pb[2:-1])       # (the rows next to the borders reflect, not wrap)


# ------------------------------------------------------------------ the engine's mapping
@pytest.mark.parametrize('rate', ['field', 'frame'])
def test_batches_over_the_engines_partition_concatenate_to_the_whole_clip(rate):
    from tecogan_pytorch_amd.models.networks.frnet_infer import clip_batches
    from tecogan_pytorch_amd.models.networks.stream import deinterlace_input_sizes, deinterlace_window
    h, w, step = 8, 10, 1 if rate == 'field' else 2
    for n in range(1, 13):
        clip = noise(n, h, w, '420', seed=n)
        whole = R.stream(clip, h, w, rate=rate)
        total = n * (2 if rate == 'field' else 1)
        assert whole.shape[0] == total
        for first, later in ((9, 8), (2, 1), (4, 3)):
            batches, sizes, have, outs = clip_batches(total, first, later), deinterlace_input_sizes(first, later, rate), 0, []
            for i0, cnt in batches:
                lo, hi, ff = deinterlace_window(i0, cnt, rate)
                assert (lo, hi, ff) == R.window(i0, cnt, rate) and -1 <= lo < hi < n and ff in (0, 1)
                assert lo >= have - 2, 'a batch reaches at most two frames back into what earlier batches took'
                if cnt == (first if i0 == 0 else later):    # a full batch takes exactly the frames the generator names
                    assert hi + 1 - have == next(sizes)
                have = hi + 1
                outs.append(R.deinterlace(clip[lo + 1:hi + 1], h, w, prev=clip[lo] if lo >= 0 else None, first_field=ff,
                                          step=step, cnt=cnt))
            assert have == n and np.array_equal(np.concatenate(outs), whole), (n, first, later)


def test_rebatch_by_sizes_hands_out_pieces_and_empty_batches():
    import torch
    from tecogan_pytorch_amd.models.networks.stream import deinterlace_input_sizes, stream_rebatch_sizes
    assert [s for s, _ in zip(deinterlace_input_sizes(9, 8), range(4))] == [5, 4, 4, 4]
    assert [s for s, _ in zip(deinterlace_input_sizes(9, 8, 'frame'), range(3))] == [9, 8, 8]
    assert [s for s, _ in zip(deinterlace_input_sizes(2, 1), range(5))] == [1, 1, 0, 1, 0]
    parts = [('yuv', torch.arange(7).reshape(7, 1)), ('yuv', torch.arange(7, 10).reshape(3, 1))]
    got = [(b, off, None if p is None else p.reshape(-1).tolist(), full)
           for b, off, p, full in stream_rebatch_sizes(iter(parts), deinterlace_input_sizes(9, 8))]
    assert got == [(0, 0, [0, 1, 2, 3, 4], True), (1, 0, [5, 6], False), (1, 2, [7, 8], True), (2, 0, [9], False)]
    got = [(b, off, None if p is None else p.reshape(-1).tolist(), full)
           for b, off, p, full in stream_rebatch_sizes(iter(parts[1:]), deinterlace_input_sizes(2, 1))]
    assert got == [(0, 0, [7], True), (1, 0, [8], True), (2, 0, None, True), (3, 0, [9], True), (4, 0, None, True)]


# ------------------------------------------------------------------ the option and the refusals
def test_deinterlace_validates_like_the_other_options():
    from tecogan_pytorch_amd.models.networks import Deinterlace
    d = Deinterlace()
    assert (d.tff, d.rate, d.per_frame) == (True, 'field', 2) and Deinterlace(False, 'frame').per_frame == 1
    assert Deinterlace(np.bool_(False)).tff is False
    with pytest.raises(Exception):
        d.tff = False                                       # frozen
    for kw in (dict(tff=1), dict(tff='t'), dict(rate='fields'), dict(rate=None), dict(rate=2)):
        with pytest.raises(ValueError, match='Deinterlace'):
            Deinterlace(**kw)


def test_infer_stream_refusals_that_need_no_device():
    from tecogan_pytorch_amd.models.networks import Deinterlace, Yuv, Yuv420
    from tecogan_pytorch_amd.models.networks.stream import _StreamEngine
    net = SimpleNamespace(in_nc=3, scale=4)
    eng = lambda **kw: _StreamEngine(net, iter([]), 'cpu', 'rerun', **kw)
    with pytest.raises(ValueError, match='yuv'):
        eng(deinterlace=Deinterlace())
    with pytest.raises(ValueError, match='must be a Deinterlace'):
        eng(yuv=Yuv420(16, 24), deinterlace={'tff': True})
    for spec in (Yuv420(18, 24), Yuv420(17, 24), Yuv(16 + 2, 24, '420'), Yuv(15, 24, '422'), Yuv(9, 24, '444'), Yuv(2, 24, '444')):
        with pytest.raises(ValueError, match='Deinterlace: .*height'):
            eng(yuv=spec, deinterlace=Deinterlace())
    for spec in (Yuv420(16, 24), Yuv(18, 23, '422'), Yuv(6, 7, '444')):
        Deinterlace().check_source(spec)


# ------------------------------------------------------------------ y4m
def test_y4m_interlaced_headers_only_on_request():
    from tecogan_pytorch_amd.data.y4m import Y4MError, Y4MReader, parse_header
    head = b'YUV4MPEG2 W24 H16 F25:1 %s A1:1 C420mpeg2'
    for tag, code in ((b'It', 't'), (b'Ib', 'b'), (b'Ip', 'p')):
        assert parse_header(head % tag, interlaced=True)['interlace'] == code
        rd = Y4MReader(io.BytesIO(head % tag + b'\n'), interlaced=True)
        assert rd.interlace == code and rd.header['interlace'] == code
    assert parse_header(head % b'Ip')['interlace'] == 'p' and Y4MReader(io.BytesIO(head % b'Ip' + b'\n')).interlace == 'p'
    for tag in (b'It', b'Ib', b'Im'):                       # the default refuses exactly as before
        with pytest.raises(Y4MError) as e:
            parse_header(head % tag)
        assert str(e.value) == f'y4m: {tag.decode()}: interlaced material is not supported (progressive Ip only)'
        with pytest.raises(Y4MError, match='progressive Ip only'):
            Y4MReader(io.BytesIO(head % tag + b'\n'))
    with pytest.raises(Y4MError, match='Im: mixed'):
        parse_header(head % b'Im', interlaced=True)
    with pytest.raises(Y4MError, match='Ix'):
        parse_header(head % b'Ix', interlaced=True)


def test_y4m_writer_rate_scale_and_ip():
    from tecogan_pytorch_amd.data.y4m import Y4MError, Y4MWriter, parse_header, scale_rate_tag
    assert scale_rate_tag('F25:1', 2, 1) == 'F50:1' and scale_rate_tag('F30000:1001', 2, 1) == 'F60000:1001'
    assert scale_rate_tag('F0:0', 2, 1) == 'F0:0' and scale_rate_tag('F50:2', 1, 1) == 'F25:1'
    for bad in (('F25', 2, 1), ('F25:1', 0, 1), ('F25:1', 2, -1)):
        with pytest.raises(Y4MError):
            scale_rate_tag(*bad)
    for f_in, f_out in (('F25:1', 'F50:1'), ('F30000:1001', 'F60000:1001'), ('F0:0', 'F0:0')):
        hdr = parse_header(f'YUV4MPEG2 W24 H16 {f_in} It A1:1 C420mpeg2'.encode(), interlaced=True)
        buf = io.BytesIO()
        Y4MWriter(buf, 96, 64, hdr, rate_scale=(2, 1))
        assert buf.getvalue() == f'YUV4MPEG2 W96 H64 {f_out} A1:1 C420mpeg2 Ip\n'.encode()
        buf = io.BytesIO()
        Y4MWriter(buf, 96, 64, hdr)
        assert buf.getvalue() == f'YUV4MPEG2 W96 H64 {f_in} A1:1 C420mpeg2 Ip\n'.encode()
    buf = io.BytesIO()
    Y4MWriter(buf, 96, 64, None, rate_scale=(2, 1))        # no F tag: none is invented
    assert buf.getvalue() == b'YUV4MPEG2 W96 H64 C420jpeg Ip\n'


# ------------------------------------------------------------------ the flags
def test_cli_flag_refusals(tmp_path, capsys):
    from tecogan_pytorch_amd.main import parse_args
    y4m = str(tmp_path / 'in.y4m')
    open(y4m, 'wb').close()
    a = parse_args(['--mode', 'infer', '--input', y4m, '--output', '-'])
    assert (a.deinterlace, a.deinterlace_rate) == ('off', None)
    a = parse_args(['--mode', 'infer', '--input', '-', '--output', '-', '--deinterlace', 'auto', '--deinterlace-rate', 'frame'])
    assert (a.deinterlace, a.deinterlace_rate) == ('auto', 'frame')
    for order in ('tff', 'bff'):
        assert parse_args(['--mode', 'infer', '--input', y4m, '--output', '-', '--deinterlace', order]).deinterlace == order
    bad = [(['--mode', 'infer', '--input', str(tmp_path), '--output', str(tmp_path), '--deinterlace', 'auto'], 'y4m input'),
           (['--mode', 'test', '--deinterlace', 'tff'], 'y4m input'),
           (['--mode', 'infer', '--input', y4m, '--output', '-', '--deinterlace-rate', 'frame'], '--deinterlace auto'),
           (['--mode', 'infer', '--input', y4m, '--output', '-', '--deinterlace', 'off', '--deinterlace-rate', 'field'],
            '--deinterlace auto'),
           (['--mode', 'infer', '--input', y4m, '--output', '-', '--deinterlace', 'yadif'], 'invalid choice'),
           (['--mode', 'infer', '--input', y4m, '--output', '-', '--deinterlace', 'auto', '--deinterlace-rate', 'double'],
            'invalid choice')]
    for argv, why in bad:
        with pytest.raises(SystemExit):
            parse_args(argv)
        assert why in capsys.readouterr().err, argv
