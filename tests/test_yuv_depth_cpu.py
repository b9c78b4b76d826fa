"""Host side of 10- and 12-bit YUV 4:2:0 (no GPU): the 2^24 integer tables, how close the integer
output formula is to fp64 (all 2^24 colours c/255, and 2^20 uniform pixels per case), the round trip, the formula at
depth 8 against section 7e's, the y4m reader / writer at 10 and 12 bits, Yuv420's new fields, the `after` hook of
enqueue_batch and the CLI options.

Bounds.  The decision stage asserts what the issue states: never more than ONE code between the integer formula and
floor(fp64 + 0.5); the share of samples that differ at all is measured, printed, and recorded in DESIGN.md.  The round
trip's bound is derived from that: a Y, Cb or Cr code is within 1 + 0.5 codes of the exact value, so an RGB value that
comes back through the fp64 inverse is off by at most 1.5 (1/ys + k/cs) of full scale, k the inverse's largest chroma
gain row sum: B with 2(1-Kb) = 1.8556 under BT.709.  In 8-bit RGB levels, limited range: 255 * 1.5 * (1/219 + 1.8556/224)
/ 2^(d-8) = 4.92 / 2^(d-8): 1.23 at 10 bits, 0.31 at 12 (the full-range figures are smaller)."""
import ctypes as C
import io
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import yuv_depth_ref as R
from tests import yuv_planar_ref as P
from tests import yuv_ref as R8
from tests.test_yuv_cpu import TABLES as TABLES_8
from tecogan_pytorch_amd import _lib as L
from tecogan_pytorch_amd.data.y4m import Y4MError, Y4MReader, Y4MWriter, frame_bytes
from tecogan_pytorch_amd.models.base_model import front_pad_stream
from tecogan_pytorch_amd.models.networks import Yuv420, yuv420_planes
from tecogan_pytorch_amd.models.networks import frnet_infer as F
from tecogan_pytorch_amd.models.networks import tecogan_nets as N
from tecogan_pytorch_amd.models.networks.stream import Resize

DEPTH_CONFIGS = [(d, m, fr) for d in R.DEPTHS for (m, fr) in R.CONFIGS]
ALL_CONFIGS = [(d, m, fr) for d in P.DEPTHS for (m, fr) in P.CONFIGS]           # 3 depths x 3 matrices x 2 ranges


def round_trip_bound(depth):
    """See the module docstring: RGB levels of 8 bits."""
    return 255.0 * 1.5 * (1 / 219.0 + 1.8556 / 224.0) / (1 << (depth - 8))


# ---------------------------------------------------------------- tables
def _reference_table(depth, matrix, full):
    """(computed from Kr and Kb, pinned) by the specification that owns the combination: section 7e's at 8 bits, section
    7k's at 10 and 12, section 7l's for BT.2020."""
    if matrix == 'bt2020':
        return P.q_table(depth, matrix, full), P.BT2020_TABLES[(depth, full)]
    if depth == 8:
        return R8.q_table(matrix, full), TABLES_8[(matrix, full)]
    return R.q_table(depth, matrix, full), R.TABLES[(depth, matrix, full)]


@pytest.mark.parametrize('depth,matrix,full', ALL_CONFIGS)
def test_q_tables_follow_from_kr_and_kb_and_are_the_kernels(depth, matrix, full):
    """What the library hands to its kernels (tg_yuv_tables: forward_table and inverse_table, no device call) against the
    three specifications, all 18 combinations."""
    t, pinned = _reference_table(depth, matrix, full)
    assert t.tolist() == pinned
    q, f = (C.c_int * 12)(), (C.c_float * 5)()
    L.check(L.lib().tg_yuv_tables(depth, L.YUV_PLANAR_MATRIX[matrix], int(full), q, f), 'tg_yuv_tables')
    yo, ys, cs, mid = P.scales(depth, full)
    assert [list(q[0:3]), list(q[3:6]), list(q[6:9])] == t.tolist()
    assert list(q[9:12]) == [yo, mid, (1 << depth) - 1]
    # the five gains of the input direction: the fp64 expressions, rounded once to fp32
    kr, kb = P.KR_KB[matrix]
    kg, cs16 = 1.0 - kr - kb, 16.0 * cs
    want = np.array([1.0 / ys, 2.0 * (1.0 - kr) / cs16, -(2.0 * kb * (1.0 - kb) / kg) / cs16,
                     -(2.0 * kr * (1.0 - kr) / kg) / cs16, 2.0 * (1.0 - kb) / cs16], np.float64).astype(np.float32)
    assert np.array_equal(np.array(list(f), np.float32), want)      # ky, rv, gu, gv, bu
    if depth == 8:
        # 8 taps of 255 at most (4:2:0, left) and the rounding term fit the 32-bit accumulator
        assert int(np.abs(t).sum(1).max()) * 8 * 255 + (128 << 19) + (1 << 18) < 2 ** 31
    else:
        # every sum fits the 64-bit accumulator with room to spare, and not a 32-bit one
        assert int(np.abs(t).sum(1).max()) * 8 * 65535 + (4096 << 27) < 2 ** 62
        assert int(t[0].sum()) * 65535 > 2 ** 31


@pytest.mark.parametrize('bad', [(9, 0, 0), (16, 1, 1), (8, 3, 0), (10, -1, 0), (12, 2, 2), (8, 0, -1)])
def test_the_table_query_refuses_what_no_kernel_takes(bad):
    q, f = (C.c_int * 12)(), (C.c_float * 5)()
    assert L.lib().tg_yuv_tables(*bad, q, f) == L.lib().tg_yuv_tables(8, 0, 0, None, f) == \
        L.lib().tg_yuv_tables(8, 0, 0, q, None) == L.TG_E_ARG
    assert list(q) == [0] * 12 and list(f) == [0.0] * 5


def test_scales_at_depth_8_are_section_7e_s():
    for full in (False, True):
        yo, ys, cs, mid = R.scales(8, full)
        assert (yo, ys, cs) == R8.scales(full) and mid == 128
    assert R.scales(10, False) == (64, 876.0, 896.0, 512) and R.scales(12, True) == (0, 4095.0, 4095.0, 2048)


def test_the_float_step_clamps_orders_nan_to_zero_and_rounds_half_even():
    v = np.array([-1.0, -0.0, 0.0, 1.0, 1.5, np.nan, np.inf, -np.inf, 0.5], np.float32)
    assert R.quantize16(v).tolist() == [0, 0, 0, 65535, 65535, 0, 65535, 0, 32768]            # 32767.5 -> even
    ties = ((np.arange(0, 2000, dtype=np.float64) + 0.5) / 65535.0).astype(np.float32)
    prod = ties * np.float32(65535.0)
    exact = prod == np.floor(prod) + np.float32(0.5)                 # the fp32 product lands on k + 0.5 exactly
    assert exact.sum() > 100
    q = R.quantize16(ties[exact])
    assert (q % 2 == 0).all() and (np.abs(q - prod[exact].astype(np.float64)) == 0.5).all()


# ---------------------------------------------------------------- decision stage
def _axis_codes():
    """c / 255 in fp32 for c = 0 .. 255: (the value as fp64 in 16-bit codes, the integer code the float step gives)."""
    v = (np.arange(256, dtype=np.float32) / np.float32(255.0)).astype(np.float32)
    q = R.quantize16(v)
    assert (q == 257 * np.arange(256)).all()
    return v.astype(np.float64) * 65535.0, q


def _separable(rows, r, g, b):
    """sum_k rows[k] * (r, g, b)[k] over the whole (256,256,256) cube, for each of the three rows: (3, 256,256,256)."""
    return np.stack([row[0] * r[:, None, None] + row[1] * g[None, :, None] + row[2] * b[None, None, :] for row in rows])


@pytest.mark.parametrize('depth,matrix,full', DEPTH_CONFIGS)
def test_integer_formula_against_fp64_over_all_colours(depth, matrix, full):
    """Constant-colour blocks (every siting reduces to the 24-bit shift), all 2^24 colours c/255; both sides clipped to
    the output's range.  The fp64 side takes the value itself, not the 16-bit code."""
    x, q = _axis_codes()
    yo, _, _, mid = R.scales(depth, full)
    top = (1 << depth) - 1
    qt, m = R.q_table(depth, matrix, full), R.forward_matrix(depth, matrix, full)
    slab = np.stack(np.meshgrid(q[::5], q[::3], q[::7], indexing='ij'), -1).reshape(-1, 3)
    slab_ycc = R.codes_to_ycc_int(slab, depth, matrix, full)
    differing, worst = np.zeros(3, np.int64), 0
    for k, off in enumerate((yo, mid, mid)):                        # one plane, 32 values of R at a time
        for r0 in range(0, 256, 32):
            rs = slice(r0, r0 + 32)
            got = np.clip((_separable(qt[k:k + 1], q[rs], q, q)[0] + (off << R.SHIFT) + (1 << (R.SHIFT - 1))) >> R.SHIFT,
                          0, top)
            ref = np.clip(np.floor(_separable(m[k:k + 1], x[rs], x, x)[0] + off + 0.5), 0, top).astype(np.int64)
            d = np.abs(got - ref)
            differing[k] += int((d != 0).sum())
            worst = max(worst, int(d.max()))
            # the two forms of the formula in the reference agree
            pick = np.arange(0, 256, 5)
            pick = pick[(pick >= r0) & (pick < r0 + 32)]
            assert np.array_equal(slab_ycc[:, k].reshape(52, 86, 37)[pick // 5], got[pick - r0][:, ::3, ::7])
    share = (differing / float(1 << 24)).tolist()
    print('depth', depth, matrix, 'full' if full else 'limited', 'differing share per plane', share, 'worst', worst)
    assert worst <= 1


@pytest.mark.parametrize('depth,siting,matrix,full', R.CASES)
def test_integer_formula_against_fp64_over_uniform_floats(depth, siting, matrix, full):
    """2^20 seeded uniform pixels as a 1024 x 1024 frame: Y per pixel, chroma per 2x2 block with the siting's weights.
    The fp64 side works on the float values themselves (times 65535), never on the rounded codes."""
    rgb = np.random.default_rng(1000 * depth + 10 * R.SITINGS.index(siting) + R.CONFIGS.index((matrix, full))) \
        .random((1, 3, 1024, 1024), dtype=np.float32)
    got = R.rgb_f32_to_yuv420p(rgb, depth, matrix, full, siting).astype(np.int64)
    y, u, v = R.planes(got, 1024, 1024)
    m = R.forward_matrix(depth, matrix, full)
    yo, _, _, mid = R.scales(depth, full)
    top = (1 << depth) - 1
    x = rgb.astype(np.float64).transpose(0, 2, 3, 1) * 65535.0
    rows = x[:, 0::2] + x[:, 1::2]
    if siting == 'center':
        s = (rows[:, :, 0::2] + rows[:, :, 1::2]) / 4.0
    else:
        left = np.concatenate([rows[:, :, :1], rows[:, :, 1:-1:2]], 2)
        s = (left + 2 * rows[:, :, 0::2] + rows[:, :, 1::2]) / 8.0
    rnd = lambda e: np.clip(np.floor(e + 0.5), 0, top).astype(np.int64)
    worst, shares = 0, []
    for name, g, ref in (('Y', y, rnd(x @ m[0] + yo)), ('Cb', u, rnd(s @ m[1] + mid)), ('Cr', v, rnd(s @ m[2] + mid))):
        d = np.abs(g - ref)
        worst = max(worst, int(d.max()))
        shares.append(float((d != 0).mean()))
    print('depth', depth, siting, matrix, 'full' if full else 'limited', 'differing share Y Cb Cr', shares, 'worst', worst)
    assert worst <= 1


# ---------------------------------------------------------------- round trip, and depth 8 against section 7e
@pytest.mark.parametrize('depth,matrix,full', DEPTH_CONFIGS)
def test_constant_colour_round_trip_over_all_colours(depth, matrix, full):
    _, q = _axis_codes()
    worst = 0.0
    gb = np.stack(np.meshgrid(q, q, indexing='ij'), -1).reshape(-1, 2)
    levels = gb // 257
    for r in range(0, 256):
        codes = np.concatenate([np.full((65536, 1), q[r]), gb], 1)
        ycc = R.codes_to_ycc_int(codes, depth, matrix, full)
        back = R.ycc_to_rgb_f64(ycc[:, 0], ycc[:, 1] * 16, ycc[:, 2] * 16, depth, matrix, full) * 255.0   # (3, 65536)
        worst = max(worst, float(np.abs(back[0] - r).max()), float(np.abs(back[1:].T - levels).max()))
    print('depth', depth, matrix, 'full' if full else 'limited', 'round trip worst %.4f RGB levels' % worst,
          'bound %.4f' % round_trip_bound(depth))
    assert worst <= round_trip_bound(depth)


@pytest.mark.parametrize('matrix,full', R.CONFIGS)
def test_depth_8_luma_is_section_7e_s_within_one_code(matrix, full):
    """The new formula at depth 8 on q = 257 c against the 16.16 formula on c, all 2^24 colours."""
    _, q = _axis_codes()
    c = np.arange(256, dtype=np.int64)
    yo = R.scales(8, full)[0]
    worst, differing = 0, 0
    for r0 in range(0, 256, 32):
        rs = slice(r0, r0 + 32)
        new = np.clip((_separable(R.q_table(8, matrix, full)[:1], q[rs], q, q)[0] + (yo << 24) + (1 << 23)) >> 24, 0, 255)
        old = np.clip((_separable(R8.q_table(matrix, full)[:1], c[rs], c, c)[0] + (yo << 16) + (1 << 15)) >> 16, 0, 255)
        d = np.abs(new - old)
        worst, differing = max(worst, int(d.max())), differing + int((d != 0).sum())
    print(matrix, 'full' if full else 'limited', 'largest difference', worst, 'share', differing / float(1 << 24))
    assert worst <= 1


def test_input_reference_at_mid_grey_and_above_the_top_code():
    for depth in R.DEPTHS:
        top, (yo, ys, _, mid) = (1 << depth) - 1, R.scales(depth, False)
        n = R.frame_samples(3, 5)
        grey = np.concatenate([np.full(15, yo + int(ys) // 2), np.full(n - 15, mid)]).astype(np.uint16)[None]
        out = R.yuv420p_to_rgb(grey, 3, 5, depth, 'bt709', False, 'left')
        assert out.shape == (1, 3, 3, 5) and np.allclose(out, (int(ys) // 2) / ys, atol=1e-12)
        over = np.full((1, n), 65535, np.uint16)
        assert np.array_equal(R.yuv420p_to_rgb(over, 3, 5, depth, 'bt601', True, 'center'),
                              R.yuv420p_to_rgb(np.full((1, n), top, np.uint16), 3, 5, depth, 'bt601', True, 'center'))


# ---------------------------------------------------------------- y4m
def _clip16(n, h, w, depth, seed=0):
    return np.random.default_rng(seed).integers(0, 1 << depth, (n, R.frame_samples(h, w)), dtype=np.uint16)


def _y4m(header, frames):
    return header + b''.join(b'FRAME\n' + f.tobytes() for f in frames)


@pytest.mark.parametrize('tag', ['C420paldv', 'C422', 'C444', 'Cmono', 'C420p10', 'C420p12', 'C420p16', 'C444p10',
                                 'It', 'Ib', 'Im'])
def test_default_reader_refuses_what_it_refused_and_names_the_tag(tag):
    with pytest.raises(Y4MError, match=tag) as e:
        Y4MReader(io.BytesIO(b'YUV4MPEG2 W4 H2 F25:1 ' + tag.encode() + b'\n'))
    if tag.startswith('C'):
        assert str(e.value).endswith('(supported: C420jpeg, C420mpeg2, C420)')


@pytest.mark.parametrize('tag', ['C420paldv', 'C422', 'C444', 'Cmono', 'C420p16', 'C420p14', 'C444p10', 'C422p10', 'C444p12',
                                 'It', 'Ib', 'Im'])
def test_reader_opened_for_all_depths_still_refuses_the_rest(tag):
    with pytest.raises(Y4MError, match=tag):
        Y4MReader(io.BytesIO(b'YUV4MPEG2 W4 H2 F25:1 ' + tag.encode() + b'\n'), depths=(8, 10, 12))
    with pytest.raises(Y4MError, match='C420p12'):
        Y4MReader(io.BytesIO(b'YUV4MPEG2 W4 H2 C420p12\n'), depths=(8, 10))


@pytest.mark.parametrize('depth', [10, 12])
def test_high_depth_headers_frames_and_short_reads(depth):
    frames = _clip16(3, 6, 10, depth, seed=depth)
    head = b'YUV4MPEG2 W10 H6 F30000:1001 Ip A1:1 C420p%d XYSCSS=420P%d XCOLORRANGE=LIMITED\n' % (depth, depth)
    data = _y4m(head, frames)
    rd = Y4MReader(io.BytesIO(data), depths=(8, 10, 12))
    assert (rd.w, rd.h, rd.depth, rd.siting, rd.full_range) == (10, 6, depth, None, False)
    assert rd.frame_bytes == 2 * 90 == frame_bytes(6, 10, depth) and rd.header['depth'] == depth
    got = [f.copy() for f in rd]
    assert len(got) == 3 and all(g.dtype == np.uint8 and np.array_equal(g.view(np.uint16), f) for g, f in zip(got, frames))

    class Dribble(io.BytesIO):                                      # every read comes back short
        def readinto(self, b):
            return super().readinto(memoryview(b)[:7])
    assert all(np.array_equal(g.view(np.uint16), f) for g, f in zip([f.copy() for f in Y4MReader(Dribble(data), (8, 10, 12))],
                                                                    frames))
    cut = Y4MReader(io.BytesIO(data[:-3]), depths=(8, 10, 12))
    next(cut), next(cut)
    with pytest.raises(Y4MError, match='ends inside frame 2'):
        next(cut)
    # 8-bit streams through the same reader: as before
    rd8 = Y4MReader(io.BytesIO(b'YUV4MPEG2 W10 H6 C420mpeg2\n'), depths=(8, 10, 12))
    assert (rd8.depth, rd8.siting, rd8.frame_bytes) == (8, 'left', 90)


def test_writer_reader_round_trip_and_tags():
    src = Y4MReader(io.BytesIO(b'YUV4MPEG2 W10 H6 F25:1 Ip A1:1 C420mpeg2 XYSCSS=420MPEG2 XCOLORRANGE=FULL\n'))
    frames = _clip16(2, 24, 40, 10, seed=3)
    out = io.BytesIO()
    wr = Y4MWriter(out, 40, 24, src.header, depth=10)
    assert wr.frame_bytes == 2 * 1440
    wr.write(frames[0])                                             # uint16 samples
    wr.write(frames[1].view(np.uint8))                              # or their bytes
    with pytest.raises(Y4MError, match='bytes'):
        wr.write(frames[0].view(np.uint8)[:1440])
    wr.flush()
    assert out.getvalue().split(b'\n', 1)[0] == b'YUV4MPEG2 W40 H24 F25:1 A1:1 C420p10 XYSCSS=420P10 XCOLORRANGE=FULL Ip'
    back = Y4MReader(io.BytesIO(out.getvalue()), depths=(8, 10, 12))
    assert (back.w, back.h, back.depth, back.siting, back.full_range) == (40, 24, 10, None, True)
    assert all(np.array_equal(g.view(np.uint16), f) for g, f in zip([f.copy() for f in back], frames)) and back.frames_read == 2
    with pytest.raises(Y4MError, match='C420p10'):
        Y4MReader(io.BytesIO(out.getvalue()))
    head = lambda **kw: (lambda o: (Y4MWriter(o, 8, 4, **kw), o.getvalue())[1])(io.BytesIO())
    assert head(header_of_input=None, depth=12) == b'YUV4MPEG2 W8 H4 C420p12 XYSCSS=420P12 Ip\n'
    assert head(header_of_input={'tags': ['F25:1']}, depth=12) == b'YUV4MPEG2 W8 H4 F25:1 C420p12 XYSCSS=420P12 Ip\n'
    assert head(header_of_input=back.header, depth=12) == \
        b'YUV4MPEG2 W8 H4 F25:1 A1:1 C420p12 XYSCSS=420P12 XCOLORRANGE=FULL Ip\n'
    # down to 8 bits: the siting names the tag, and is needed
    assert head(header_of_input=back.header, depth=8, siting='left') == \
        b'YUV4MPEG2 W8 H4 F25:1 A1:1 C420mpeg2 XYSCSS=420MPEG2 XCOLORRANGE=FULL Ip\n'
    with pytest.raises(Y4MError, match='siting'):
        head(header_of_input=back.header, depth=8)
    with pytest.raises(Y4MError, match='depth'):
        head(header_of_input=None, depth=16)
    # depth 8 after an 8-bit input: byte for byte what it was
    assert head(header_of_input=src.header) == head(header_of_input=src.header, depth=8, siting='center') == \
        b'YUV4MPEG2 W8 H4 F25:1 A1:1 C420mpeg2 XYSCSS=420MPEG2 XCOLORRANGE=FULL Ip\n'


# ---------------------------------------------------------------- Yuv420, the stream's host logic
def test_yuv420_depth_fields_and_byte_counts():
    spec = Yuv420(9, 11)
    assert (spec.depth, spec.out_depth, spec.od) == (8, None, 8) and spec == Yuv420(9, 11, depth=8)
    assert spec.frame_bytes == 159 and spec.out_frame_bytes(4) == 36 * 44 * 3 // 2
    for d_in, d_out, od in ((8, 10, 10), (10, None, 10), (10, 10, 10), (12, 8, 8), (12, 12, 12), (10, 12, 12), (8, 8, 8)):
        s = Yuv420(9, 11, depth=d_in, out_depth=d_out)
        assert s.od == od
        assert s.frame_bytes == 159 * (2 if d_in > 8 else 1)
        assert s.out_frame_bytes(4) == 36 * 44 * 3 // 2 * (2 if od > 8 else 1)
        assert s.out_frame_bytes(2) == 18 * 22 * 3 // 2 * (2 if od > 8 else 1)
    assert Yuv420(9, 11, depth=10) != Yuv420(9, 11) and hash(Yuv420(9, 11, out_depth=10)) == hash(Yuv420(9, 11, out_depth=10))
    assert Yuv420(9, 11, depth=np.int64(12)).depth == 12
    for bad in (dict(depth=9), dict(depth=16), dict(depth=None), dict(depth=10.0), dict(depth=True), dict(out_depth=14),
                dict(out_depth='10'), dict(out_depth=False)):
        with pytest.raises(ValueError, match='Yuv420'):
            Yuv420(8, 8, **bad)


def test_resize_with_a_deep_output_is_refused_before_anything_is_pulled():
    net = N.FRNet(3, 3, 64, 10, 'BD', 4)
    pulled = []

    def items():
        pulled.append(1)
        yield np.zeros(Yuv420(8, 8).frame_bytes, np.uint8)
    for spec in (Yuv420(8, 8, out_depth=10), Yuv420(8, 8, depth=12)):
        with pytest.raises(ValueError, match='8-bit'):
            net.infer_stream(items(), device='cpu', yuv=spec, resize=Resize(16, 16))
    assert pulled == []
    from tecogan_pytorch_amd.models.networks import Png
    with pytest.raises(ValueError, match='png and yuv'):
        net.infer_stream(items(), device='cpu', yuv=Yuv420(8, 8, out_depth=10), png=Png())
    assert list(net.infer_stream(iter([]), device='cpu', yuv=Yuv420(8, 8, depth=10, out_depth=12))) == []


def test_stream_parts_takes_bytes_or_samples_of_deep_frames():
    spec = Yuv420(6, 10, depth=10)
    fb = spec.frame_bytes
    assert fb == 180
    clip = _clip16(4, 6, 10, 10, seed=2)
    ok = [clip[0], clip[1].view(np.uint8), torch.from_numpy(clip[2:4].view(np.uint8).copy()), clip[2:4],
          torch.from_numpy(clip[3].copy()), np.zeros((0, fb), np.uint8)]
    parts = list(N.stream_parts(iter(ok), 3, spec))
    assert [(k, tuple(x.shape), x.dtype) for k, x in parts] == [('yuv', (n, fb), torch.uint8) for n in (1, 1, 2, 2, 1)]
    want = [clip[0:1], clip[1:2], clip[2:4], clip[2:4], clip[3:4]]
    assert all(np.array_equal(x.numpy().view(np.uint16), w) for (_, x), w in zip(parts, want))
    for bad in (np.zeros(fb // 2, np.uint8), np.zeros(fb, np.uint16), np.zeros(fb // 2, np.int16), np.zeros(fb // 2, np.float32),
                np.zeros((6, 10, 3), np.uint8)):
        with pytest.raises(ValueError, match='infer_stream'):
            list(N.stream_parts(iter([bad]), 3, spec))
    with pytest.raises(ValueError, match='infer_stream'):           # an 8-bit stream takes no uint16 items
        list(N.stream_parts(iter([np.zeros(90, np.uint16)]), 3, Yuv420(6, 10)))
    # front padding: longer items, the same code
    got = torch.cat(list(front_pad_stream(iter([f for f in clip]), 'reflect', 2, 3, spec)), 0)
    assert np.array_equal(got.numpy().view(np.uint16), np.concatenate([clip[1:3][::-1], clip], 0))


def test_yuv420_planes_views_deep_chunks_as_uint16():
    clip = _clip16(3, 6, 10, 12, seed=4)
    for chunk in (clip.view(np.uint8), clip, torch.from_numpy(clip.view(np.uint8).copy())):
        y, u, v = yuv420_planes(chunk, 6, 10, depth=12)
        assert tuple(y.shape) == (3, 6, 10) and tuple(u.shape) == tuple(v.shape) == (3, 3, 5)
        assert y.dtype in (np.uint16, torch.uint16)
        y, u, v = (np.asarray(p) if isinstance(p, np.ndarray) else p.numpy() for p in (y, u, v))
        assert np.array_equal(np.concatenate([p.reshape(3, -1) for p in (y, u, v)], 1), clip)
    y, _, _ = yuv420_planes(clip.view(np.uint8), 6, 10, depth=12)
    assert np.shares_memory(y, clip)
    y1, u1, _ = yuv420_planes(clip[0].view(np.uint8), 6, 10, 10)
    assert y1.shape == (6, 10) and u1.shape == (3, 5)
    with pytest.raises(ValueError):
        yuv420_planes(clip.view(np.uint8), 6, 10)                   # twice the bytes of an 8-bit frame
    with pytest.raises(ValueError):
        yuv420_planes(clip.view(np.uint8)[:, :90], 6, 10, depth=10)
    with pytest.raises(ValueError):
        yuv420_planes(clip, 6, 10, depth=9)


# ---------------------------------------------------------------- enqueue_batch's `after` hook (a recording fake)
class _Lib:
    def __init__(self, trace):
        self.trace = trace

    def tg_frnet_step_srnet(self, *a):
        self.trace.append(('srnet', a[4]))                          # the HR state the launch writes
        return 0

    def tg_frnet_step_phase(self, *a):
        self.trace.append(('phase',))
        return 0

    def tg_zero_if_flag(self, *a):
        self.trace.append(('zero', a[0]))
        return 0

    def tg_frnet_plan_flow(self, *a):
        return 1 << 28


class _Stream:
    cuda_stream = 11

    def wait_event(self, ev):
        pass


def _run_batches(t, first, later, with_after, reset=None):
    trace, hr = [], (50000, 60000)
    ev = SimpleNamespace(record=lambda s: None)
    for b, (i0, cnt) in enumerate(F.clip_batches(t, first, later)):
        after = (lambda j, addr, i0=i0: trace.append(('after', i0 + j, addr))) if with_after else None
        F.enqueue_batch(_Lib(trace), SimpleNamespace(handle=1), lambda n: SimpleNamespace(handle=2), b, i0, cnt, 1 << 20,
                        1000, hr, 1 << 24, 300, 42, 64, _Stream(), _Stream(), ev, ev, reset=reset, after=after)
    return trace, hr


@pytest.mark.parametrize('t', [1, 2, 10, 19])
def test_after_runs_directly_behind_every_frame_with_the_state_just_written(t):
    for reset in (None, (7000, 4096)):
        trace, hr = _run_batches(t, 3, 2, True, reset)
        plain, _ = _run_batches(t, 3, 2, False, reset)
        assert [e for e in trace if e[0] != 'after'] == plain       # nothing else moves
        at = [k for k, e in enumerate(trace) if e[0] == 'after']
        assert [trace[k][1] for k in at] == list(range(t))           # every frame once, in order, frame 0 included
        for k in at:
            i = trace[k][1]
            assert trace[k - 1] == ('srnet', hr[(i + 1) & 1]) and trace[k][2] == hr[(i + 1) & 1]


# ---------------------------------------------------------------- the CLI options
def test_cli_depth_and_siting_options(tmp_path):
    from tecogan_pytorch_amd import main as M
    y4m = tmp_path / 'clip.y4m'
    y4m.write_bytes(b'YUV4MPEG2 W4 H2 C420p10\n')
    folder = str(tmp_path)
    a = M.parse_args(['--mode', 'infer', '--input', str(y4m), '--output', '-'])
    assert (a.output_depth, a.yuv_siting) == (None, 'left')
    a = M.parse_args(['--mode', 'infer', '--input', '-', '--output', '-', '--output-depth', '10', '--yuv-siting', 'center'])
    assert (a.output_depth, a.yuv_siting) == (10, 'center')
    assert M.parse_args(['--mode', 'infer', '--input', str(y4m), '--output-depth', '8', '--output-size', '8x4']).output_depth == 8
    for bad in (['--mode', 'infer', '--input', folder, '--output-depth', '10'],            # a PNG folder
                ['--mode', 'infer', '--output-depth', '10'],                               # no input at all
                ['--mode', 'test', '--input', str(y4m), '--output-depth', '10'],
                ['--mode', 'infer', '--input', str(y4m), '--output-depth', '9'],
                ['--mode', 'infer', '--input', str(y4m), '--output-depth', '16'],
                ['--mode', 'infer', '--input', str(y4m), '--output-depth', '12', '--output-size', '8x4'],
                ['--mode', 'infer', '--input', str(y4m), '--yuv-siting', 'topleft']):
        with pytest.raises(SystemExit) as e:
            M.parse_args(bad)
        assert e.value.code == 2, bad
