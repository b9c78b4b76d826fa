"""CPU: the bicubic resize to any size.  The specification tests/resize_ref.py against the BI
tables and bytes it generalises, against the fp64 route of the same algorithm and against torch's antialiased bicubic;
ops.resample_tables against the specification; the bounds the kernel's buffers rely on; and the host side of the
stream option, the y4m A tag and the command line.  No kernel is launched here."""
import io
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import bi_ref as B
from tests import resize_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (h_in, w_in, h_out, w_out) of every case tests/test_hip_resize.py runs
GPU_SHAPES = [(8, 8, 2, 2), (5, 7, 20, 28), (37, 53, 41, 29), (48, 64, 27, 36), (150, 290, 67, 131), (64, 96, 36, 54),
              (16, 24, 8, 12), (16, 24, 4, 6), (134, 262, 67, 131), (268, 524, 67, 131), (9, 5, 3, 20), (64, 96, 16, 24),
              (64, 96, 36, 48), (16, 16, 8, 8), (300, 300, 80, 80)]
# the shapes the issue sets for the comparison with the second formulations
FLOAT_SHAPES = [(48, 64, 27, 36), (64, 96, 36, 54), (40, 60, 90, 135), (37, 53, 41, 29), (64, 64, 16, 256)]


def _axis_pairs(limit):
    return [(a, b) for a in range(1, limit + 1) for b in range(-(-a // 4), 4 * a + 1)]


def test_every_row_sums_to_one_and_the_bounds_of_the_accumulators_hold():
    """2^14 per row exactly; the taps fit MAX_TAPS; sum |q| stays below 1.3 x 2^14, so the vertical partial sum
    (255 sum |q| < 2^23) fits int32 and |N| <= 255 (sum |q|)^2 needs 64 bits."""
    worst = 0
    for a, b in _axis_pairs(48) + [(a, b) for a in (97, 268, 536, 1280) for b in (a // 4 + 1, a // 2 + 3, 2 * a + 1)]:
        idx, q = R.tables(a, b)
        assert idx.dtype == np.int32 and q.dtype == np.int16 and idx.shape == q.shape == (b, q.shape[1])
        assert q.shape[1] <= R.MAX_TAPS
        assert np.all(q.astype(np.int64).sum(axis=1) == R.ONE), (a, b)
        assert idx.min() >= 0 and idx.max() <= a - 1
        worst = max(worst, int(np.abs(q.astype(np.int64)).sum(axis=1).max()))
    assert R.ONE < worst < 1.3 * R.ONE
    assert 255 * worst * worst > 2 ** 32


@pytest.mark.parametrize('s', [2, 4])
def test_tables_at_one_half_and_one_quarter_are_the_bi_tables(s):
    """For n from s to 67 s the integer weights are bi_ref.WEIGHTS[s] times 2^14 / DENOM[s] (64 and 4) with no
    residual, and the indices are the BI taps."""
    factor = R.ONE // B.DENOM[s]
    assert factor * B.DENOM[s] == R.ONE and factor == {2: 64, 4: 4}[s]
    for m in range(1, 68):
        idx, q = R.tables(s * m, m)
        assert q.shape == (m, 4 * s)
        assert np.array_equal(q.astype(np.int64), np.broadcast_to(B.WEIGHTS[s] * factor, (m, 4 * s))), (s, m)
        assert np.array_equal(idx.astype(np.int64), B.tap_indices(s * m, s)), (s, m)


@pytest.mark.parametrize('s', [2, 4])
def test_specification_equals_the_bi_degradation(s):
    rs = np.random.RandomState(5 + s)
    for h, w in [(s, 2 * s), (5 * s, 7 * s), (16 * s, 24 * s)]:
        x = rs.randint(0, 256, (2, h, w, 3)).astype(np.uint8)
        x[0, : h // 2] = (x[0, : h // 2] > 127) * 255
        assert np.array_equal(R.resize_u8(x, h // s, w // s), B.bi_downsample_u8(x, s))
        assert np.array_equal(R.exact_sums(x, h // s, w // s), B.exact_sums(x, s) * (R.ONE // B.DENOM[s]) ** 2)


def test_ops_tables_equal_the_specification():
    from tecogan_pytorch_amd import ops
    pairs = {(s[0], s[2]) for s in GPU_SHAPES + FLOAT_SHAPES} | {(s[1], s[3]) for s in GPU_SHAPES + FLOAT_SHAPES}
    pairs |= set(_axis_pairs(24)) | {(536, 402), (1280, 960), (536, 268), (1280, 640), (1080, 4320), (4320, 1080)}
    for a, b in sorted(pairs):
        gi, gq = ops.resample_tables(a, b)
        ri, rq = R.tables(a, b)
        assert gi.dtype == np.int32 and gq.dtype == np.int16 and gi.flags.c_contiguous and gq.flags.c_contiguous
        assert gi.shape == ri.shape and np.array_equal(gi, ri) and np.array_equal(gq, rq), (a, b)
    assert (ops.RESAMPLE_MAX_TAPS, ops.RESAMPLE_WEIGHT_BITS) == (R.MAX_TAPS, R.WEIGHT_BITS)
    for a, b in [(0, 1), (1, 0), (9, 2), (2, 9), (-4, -4)]:
        with pytest.raises(RuntimeError):
            ops.resample_tables(a, b)
        with pytest.raises(ValueError):
            R.tables(a, b)


def test_a_tile_of_the_kernel_reads_no_more_than_it_can_stage():
    """The kernel stages min .. max of the indices of a tile's RS_TH (RS_TW) table rows, in LDS the host sizes by
    tg_resample_tile_span = (tile - 1) ceil(n_in / n_out) + taps + 2 (never more than n_in, nor than the caps RS_RH /
    RS_CW, which hold the ratio 1/4 with 18 taps).  Tiles start at multiples of the tile size."""
    from tecogan_pytorch_amd import _lib as L
    span = L.lib().tg_resample_tile_span
    src = open(os.path.join(ROOT, 'tecogan-pytorch_amd', 'csrc', 'tg_resize.hip')).read()
    k = {m.group(1): int(m.group(2)) for m in re.finditer(r'\b(RS_TH|RS_TW|RS_RH|RS_CW) = (\d+)', src)}
    assert set(k) == {'RS_TH', 'RS_TW', 'RS_RH', 'RS_CW'}
    for tile, cap in ((k['RS_TH'], k['RS_RH']), (k['RS_TW'], k['RS_CW'])):
        assert span(4000, 1000, R.MAX_TAPS, tile) == (tile - 1) * 4 + R.MAX_TAPS + 2 <= cap
    assert span(7, 28, 6, 8) == 7 and span(37, 41, 6, 8) == 15 and span(0, 1, 6, 8) == span(5, 5, 0, 8) == -1
    sizes = [(a, b) for a in range(1, 141) for b in sorted({-(-a // 4), -(-a // 4) + 1, a // 3 + 1, a // 2 + 1, a,
                                                             (3 * a) // 4 + 1, 2 * a + 1, 4 * a})
             if 4 * b >= a and b <= 4 * a]
    sizes += [(a, b) for a in (536, 1280, 2160) for b in (a // 4, a // 4 + 1, a // 4 + 7, (3 * a) // 4, a // 2)]
    tight = 0
    for a, b in sizes:
        idx, _ = R.tables(a, b)
        for tile in (k['RS_TH'], k['RS_TW']):
            bound = span(a, b, idx.shape[1], tile)
            for o in range(0, b, tile):
                need = int(idx[o:o + tile].max() - idx[o:o + tile].min() + 1)
                assert need <= bound, (a, b, tile, o, need, bound)
                tight = max(tight, need - bound)
    assert tight == 0                                                   # (reached: small frames are read whole)


def _torch_antialias(x_u8, h_out, w_out):
    t = torch.from_numpy(x_u8.astype(np.float64)).permute(2, 0, 1)[None]
    y = torch.nn.functional.interpolate(t, size=(h_out, w_out), mode='bicubic', align_corners=False, antialias=True)
    return np.floor(np.clip(y[0].permute(1, 2, 0).numpy(), 0.0, 255.0) + 0.5).astype(np.uint8)


@pytest.mark.parametrize('h_in,w_in,h_out,w_out', FLOAT_SHAPES)
def test_specification_against_fp64_and_torch_antialias(h_in, w_in, h_out, w_out):
    """Uniform noise.  The integer weights move a byte only where the exact value lies near k + 1/2: never more than
    one level, at no more than 1 % of the bytes (the specification gave 0.19 to 0.48 %).  torch's antialiased bicubic is
    the same kernel with the window cut at the border in place of the mirror: compared on the interior, the output
    pixels whose taps (2 max(1, n_in / n_out) input pixels to either side) stay inside the frame."""
    x = np.random.RandomState(h_in * 1000 + w_out).randint(0, 256, (h_in, w_in, 3)).astype(np.uint8)
    got = R.resize_u8(x, h_out, w_out).astype(np.int64)
    assert got.shape == (h_out, w_out, 3)
    fp = R.resize_fp64(x, h_out, w_out).astype(np.int64)
    d = np.abs(got - fp)
    print(f'{h_in}x{w_in} -> {h_out}x{w_out}: fp64 route: max {d.max()}, {100.0 * (d != 0).mean():.3f} % differ')
    assert d.max() <= 1 and (d != 0).mean() <= 0.01
    ta = _torch_antialias(x, h_out, w_out).astype(np.int64)
    my = math.ceil(2 * max(h_out / h_in, 1.0)) + 1
    mx = math.ceil(2 * max(w_out / w_in, 1.0)) + 1
    assert h_out > 2 * my and w_out > 2 * mx
    d = np.abs(got - ta)[my:-my, mx:-mx]
    print(f'{h_in}x{w_in} -> {h_out}x{w_out}: torch antialias, interior: max {d.max()}, '
          f'{100.0 * (d != 0).mean():.3f} % differ')
    assert d.max() <= 1 and (d != 0).mean() <= 0.01


def test_accumulator_pattern_needs_64_bits():
    """The frame that is 255 where the weight product is positive drives one pixel's sum past 2^32 at the ratio 1/4."""
    x = R.accumulator_pattern(64, 96, 16, 24, 7, 11)
    N = R.exact_sums(x, 16, 24)
    assert int(N[7, 11, 0]) == int(N.max()) > 2 ** 32 and int(N.min()) < 0
    y = R.resize_u8(x, 16, 24)
    assert y[7, 11, 0] == 255 and y.min() == 0


# ------------------------------------------------------------------ the stream option
def test_resize_validation():
    from tecogan_pytorch_amd.models.networks import Resize
    r = Resize(np.int64(36), 54)
    assert (r.h, r.w) == (36, 54) and type(r.h) is int and r == Resize(36, 54)
    with pytest.raises(Exception):
        r.h = 3                                                         # frozen
    for bad in [(0, 4), (4, 0), (-2, 4), (4.0, 4), ('4', 4), (True, 4), (4, None)]:
        with pytest.raises(ValueError, match='Resize'):
            Resize(*bad)
    Resize(16, 24).check_source(64, 96)                                 # 1/4
    Resize(256, 384).check_source(64, 96)                               # 4
    for h, w in [(15, 24), (16, 23), (257, 384), (256, 385)]:
        with pytest.raises(ValueError, match='ratio'):
            Resize(h, w).check_source(64, 96)


class _Counting:
    def __init__(self, items):
        self.items, self.pulled = list(items), 0

    def __iter__(self):
        return self

    def __next__(self):
        if self.pulled >= len(self.items):
            raise StopIteration
        self.pulled += 1
        return self.items[self.pulled - 1]


def test_refusals_happen_before_anything_is_pulled():
    from tecogan_pytorch_amd.models import networks as N
    net = N.FRNet(3, 3, 64, 10, 'BD', 4)
    yuv = N.Yuv420(16, 24)
    frame = np.zeros(yuv.frame_bytes, np.uint8)
    cases = [({'resize': (36, 54)}, 'Resize'),                                          # not a Resize
             ({'resize': N.Resize(35, 54), 'yuv': yuv}, 'even'),                        # odd h with yuv
             ({'resize': N.Resize(36, 53), 'yuv': yuv}, 'even'),                        # odd w with yuv
             ({'resize': N.Resize(14, 54), 'yuv': yuv}, 'ratio'),                       # below 1/4 of 64
             ({'resize': N.Resize(36, 386), 'yuv': yuv}, 'ratio')]                      # above 4 x 96
    for kw, match in cases:
        src = _Counting([frame])
        with pytest.raises(ValueError, match=match):
            net.infer_stream(src, device='cpu', **kw)
        assert src.pulled == 0
    net1 = N.FRNet(1, 1, 64, 10, 'BD', 4)
    src = _Counting([np.zeros((16, 24, 1), np.uint8)])
    with pytest.raises(ValueError, match='in_nc'):
        net1.infer_stream(src, device='cpu', resize=N.Resize(36, 54))
    assert src.pulled == 0
    # RGB items: the HR size is known when the first item shows it; refused there, before anything is allocated
    src = _Counting([np.zeros((16, 24, 3), np.uint8)] * 3)
    gen = net.infer_stream(src, device='cpu', resize=N.Resize(15, 54))
    with pytest.raises(ValueError, match='ratio'):
        next(gen)
    assert src.pulled == 1
    assert list(net.infer_stream(iter([]), device='cpu', resize=N.Resize(36, 54))) == []      # the network is free again


def test_vsr_model_passes_resize_on_and_refuses_before_a_pull():
    from tecogan_pytorch_amd.main import default_opt
    from tecogan_pytorch_amd.models import define_model
    from tecogan_pytorch_amd.models.networks import Resize, Yuv420
    opt = default_opt()
    opt.update({'is_train': False, 'dist': False, 'device': 'cpu', 'rank': 0, 'world_size': 1})
    model = define_model(opt)
    yuv = Yuv420(16, 24)
    src = _Counting([np.zeros(yuv.frame_bytes, np.uint8)] * 4)
    with pytest.raises(ValueError, match='even'):
        next(model.infer_stream(src, yuv=yuv, resize=Resize(37, 54)))
    assert src.pulled == 0


# ------------------------------------------------------------------ y4m and the command line
def test_aspect_tag_arithmetic():
    from tecogan_pytorch_amd.data.y4m import Y4MError, Y4MReader, Y4MWriter, scale_aspect_tag
    assert scale_aspect_tag('A1:1', 96 * 36, 64 * 54) == 'A1:1'                          # 64x96 -> 36x54: same shape
    assert scale_aspect_tag('A1:1', 96 * 36, 64 * 48) == 'A9:8'                          # 64x96 -> 36x48
    assert scale_aspect_tag('A4:3', 1920 * 1080, 1080 * 1440) == 'A16:9'                 # anamorphic: 1440 wide shows as 1920
    assert scale_aspect_tag('A128:117', 2, 4) == 'A64:117'
    assert scale_aspect_tag('A0:0', 9, 8) == 'A0:0'                                      # unknown stays unknown
    for tag, num, den in [('A1', 1, 1), ('Ax:y', 1, 1), ('A1:1', 0, 1), ('A1:1', 1, -1)]:
        with pytest.raises(Y4MError):
            scale_aspect_tag(tag, num, den)
    hdr = {'tags': ['F25:1', 'A1:1', 'C420jpeg', 'XCOLORRANGE=FULL']}
    plain, same, scaled = io.BytesIO(), io.BytesIO(), io.BytesIO()
    Y4MWriter(plain, 48, 36, hdr)
    Y4MWriter(same, 48, 36, hdr, aspect_scale=None)
    Y4MWriter(scaled, 48, 36, hdr, aspect_scale=(96 * 36, 64 * 48))
    assert plain.getvalue() == same.getvalue() == b'YUV4MPEG2 W48 H36 F25:1 A1:1 C420jpeg XCOLORRANGE=FULL Ip\n'
    assert scaled.getvalue() == b'YUV4MPEG2 W48 H36 F25:1 A9:8 C420jpeg XCOLORRANGE=FULL Ip\n'
    assert Y4MReader(io.BytesIO(scaled.getvalue())).header['tags'][1] == 'A9:8'
    none = io.BytesIO()
    Y4MWriter(none, 48, 36, {'tags': ['F25:1', 'C420jpeg']}, aspect_scale=(9, 8))       # no A tag: none is made up
    assert none.getvalue() == b'YUV4MPEG2 W48 H36 F25:1 C420jpeg Ip\n'


def test_parse_args_output_size():
    from tecogan_pytorch_amd.main import parse_args, resize_option
    from tecogan_pytorch_amd.models.networks import Resize
    a = parse_args(['--mode', 'infer', '--input', 'lr', '--output', 'sr', '--output-size', '3840x2160'])
    assert a.output_size == (3840, 2160) and resize_option(a.output_size) == Resize(2160, 3840)
    assert parse_args(['--mode', 'infer', '--input', 'lr', '--output', 'sr']).output_size is None
    assert resize_option(None) is None
    assert parse_args(['--mode', 'infer', '--output-size', '54X36', '--png-encoder', 'device']).output_size == (54, 36)
    for bad in ('3840', '3840x', 'x2160', '0x4', '4x0', '-4x4', '4x4x4', '4.0x4', 'WxH'):
        with pytest.raises(SystemExit):
            parse_args(['--mode', 'infer', '--output-size', bad])
    with pytest.raises(SystemExit):
        parse_args(['--mode', 'test', '--output-size', '54x36'])
