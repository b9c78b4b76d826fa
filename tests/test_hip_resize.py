"""GPU: the bicubic resize to any size (tg_resample_u8, ops.resize_u8, FRNet.infer_stream(resize=...), --output-size;
DESIGN.md section 7j) BIT FOR BIT against the integer specification tests/resize_ref.py: a halo that wraps, up- and
down-sampling, mixed ratios, several tiles with partial ones at both ends, buffers at an odd byte and nothing written
outside them; the BI degradation as the special case it is; and the stream in its three output forms."""
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

from procedural_weights import generator_state_dict, smooth_clip
from tests import png_ref as P
from tests import resize_ref as R
from tests import yuv_ref as Y
from tests.test_resize_cpu import GPU_SHAPES
from tecogan_pytorch_amd import _lib as L
from tecogan_pytorch_amd import ops

DEV = torch.device('cuda', 0)
GUARD = 0xA5
SHAPES = [(8, 8, 2, 2),                 # one tile; 16 taps on 8 pixels: the halo wraps
          (5, 7, 20, 28),               # x4 up
          (37, 53, 41, 29),             # up along one axis, down along the other
          (48, 64, 27, 36),             # 9/16
          (150, 290, 67, 131)]          # several tiles per axis, no multiple of a tile in either
_REF, _KEEP = {}, []


def _case(shape, n):
    """Input and expected bytes, made once per case and shared."""
    key = (shape, n)
    if key not in _REF:
        h_in, w_in, h_out, w_out = shape
        rs = np.random.RandomState(h_in * 31 + w_out + n)
        x = rs.randint(0, 256, (n, h_in, w_in, 3)).astype(np.uint8)
        x[0, : h_in // 2] = (x[0, : h_in // 2] > 127) * 255                   # {0, 255}: both clamps
        _REF[key] = (x, R.resize_u8(x, h_out, w_out))
    return _REF[key]


def _tables(n_in, n_out):
    idx, w, taps = ops.resample_tables_device(n_in, n_out, DEV)
    _KEEP.append((idx, w))                                                     # (the cache may drop them)
    return idx.data_ptr(), w.data_ptr(), taps


def _raw(x, h_out, w_out, in_off=0, out_off=0, pad=64, tables=None):
    """tg_resample_u8 on buffers that start in_off / out_off bytes into their allocations, the output between two
    guards of `pad` bytes: (rc, frames or None, guards intact)."""
    n, h_in, w_in, _ = x.shape
    xin = torch.empty(x.size + in_off + 8, dtype=torch.uint8, device=DEV)
    xin[in_off:in_off + x.size].copy_(torch.from_numpy(x.reshape(-1)))
    nb = n * h_out * w_out * 3
    buf = torch.full((pad + out_off + nb + pad,), GUARD, dtype=torch.uint8, device=DEV)
    vt, ht = tables or (_tables(h_in, h_out), _tables(w_in, w_out))
    rc = L.lib().tg_resample_u8(xin.data_ptr() + in_off, buf.data_ptr() + pad + out_off, n, h_in, w_in, h_out, w_out,
                                *vt, *ht, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    lo = pad + out_off
    intact = bool(np.all(host[:lo] == GUARD) and np.all(host[lo + nb:] == GUARD))
    return rc, host[lo:lo + nb].reshape(n, h_out, w_out, 3), intact


def test_the_cpu_module_checks_the_tables_of_these_shapes():
    assert set(SHAPES) <= set(GPU_SHAPES)


@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('shape', SHAPES, ids=['%dx%d-%dx%d' % s for s in SHAPES])
def test_bytes_equal_the_specification(shape, n):
    x, ref = _case(shape, n)
    got = ops.resize_u8(torch.from_numpy(x).to(DEV), shape[2:])
    assert got.dtype == torch.uint8 and tuple(got.shape) == ref.shape
    assert np.array_equal(got.cpu().numpy(), ref), int((got.cpu().numpy() != ref).sum())
    out = torch.full(ref.shape, 7, dtype=torch.uint8, device=DEV)
    assert ops.resize_u8(torch.from_numpy(x).to(DEV), shape[2:], out=out) is out
    assert np.array_equal(out.cpu().numpy(), ref)


@pytest.mark.parametrize('shape', SHAPES, ids=['%dx%d-%dx%d' % s for s in SHAPES])
def test_buffers_at_an_odd_byte_and_nothing_outside_is_written(shape):
    x, ref = _case(shape, 3)
    for in_off, out_off in ((1, 1), (3, 2), (0, 0)):
        rc, got, intact = _raw(x, shape[2], shape[3], in_off, out_off)
        assert rc == L.TG_OK and intact, (in_off, out_off)
        assert np.array_equal(got, ref), (in_off, out_off, int((got != ref).sum()))


def test_all_256_constant_frames_stay_constant():
    """Every row of a table sums to 2^14: a constant frame of value k gives k everywhere, all 256 in one launch."""
    x = np.broadcast_to(np.arange(256, dtype=np.uint8)[:, None, None, None], (256, 9, 5, 3)).copy()
    y = ops.resize_u8(torch.from_numpy(x).to(DEV), (3, 20)).cpu()
    assert torch.equal(y, torch.arange(256, dtype=torch.uint8)[:, None, None, None].expand(256, 3, 20, 3))


def test_accumulator_width():
    """x = 255 where qv[r] qh[c] > 0 for one output pixel at the ratio 1/4: its exact sum passes 2^32 (a 32-bit
    accumulate would wrap to a small byte); the specification clamps to 255."""
    x = R.accumulator_pattern(64, 96, 16, 24, 7, 11)[None]
    N = R.exact_sums(x, 16, 24)
    assert int(N[0, 7, 11, 0]) > 2 ** 32
    ref = R.resize_u8(x, 16, 24)
    assert ref[0, 7, 11, 0] == 255 and ref.min() == 0
    assert np.array_equal(ops.resize_u8(torch.from_numpy(x).to(DEV), (16, 24)).cpu().numpy(), ref)


@pytest.mark.parametrize('s', [2, 4])
def test_one_half_and_one_quarter_are_the_bi_degradation(s):
    rs = np.random.RandomState(70 + s)
    for h, w in [(16, 24), (67 * s, 131 * s)]:
        x = torch.from_numpy(rs.randint(0, 256, (2, h, w, 3)).astype(np.uint8)).to(DEV)
        assert torch.equal(ops.resize_u8(x, (h // s, w // s)), ops.downsample_bi(x, s, pad=True, out='u8'))


def _raw_zero_rows(x, vt, ht):
    """h_out = 0, which _raw cannot shape a buffer for: (rc, the untouched buffer, True)."""
    buf = torch.full((256,), GUARD, dtype=torch.uint8, device=DEV)
    xd = torch.from_numpy(x).to(DEV)
    rc = L.lib().tg_resample_u8(xd.data_ptr(), buf.data_ptr(), x.shape[0], x.shape[1], x.shape[2], 0, 8, *vt, *ht,
                                torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, buf.cpu().numpy(), True


def test_refused_calls_launch_nothing_and_set_a_message():
    x = np.full((1, 16, 16, 3), 9, np.uint8)
    lib = L.lib()
    good = (_tables(16, 8), _tables(16, 8))
    (vi, vw, vt), (hi, hw, ht) = good
    cases = [((vi, vw, 0), (hi, hw, ht), 8, 8, L.TG_E_ARG, 'taps'),
             ((vi, vw, vt), (hi, hw, 19), 8, 8, L.TG_E_ARG, 'taps'),
             ((None, vw, vt), (hi, hw, ht), 8, 8, L.TG_E_ARG, 'null'),
             ((vi, vw, vt), (hi, None, ht), 8, 8, L.TG_E_ARG, 'null'),
             ((vi, vw, vt), (hi, hw, ht), 3, 8, L.TG_E_SHAPE, 'ratio'),
             ((vi, vw, vt), (hi, hw, ht), 8, 65, L.TG_E_SHAPE, 'ratio'),
             ((vi, vw, vt), (hi, hw, ht), 0, 8, L.TG_E_SHAPE, 'size')]
    for vt_, ht_, h_out, w_out, code, word in cases:
        rc, got, intact = _raw(x, max(h_out, 1), w_out, 1, 1, tables=(vt_, ht_)) if h_out else _raw_zero_rows(x, vt_, ht_)
        assert rc == code and intact and np.all(got == GUARD), (word, rc)
        assert word in lib.tg_last_error_string().decode().lower(), (word, lib.tg_last_error_string())
    xd = torch.from_numpy(x).to(DEV)
    st = torch.cuda.current_stream().cuda_stream
    y = torch.full((1, 8, 8, 3), GUARD, dtype=torch.uint8, device=DEV)
    assert lib.tg_resample_u8(xd.data_ptr(), y.data_ptr(), 0, 16, 16, 8, 8, vi, vw, vt, hi, hw, ht, st) == L.TG_E_ARG
    assert lib.tg_resample_u8(None, y.data_ptr(), 1, 16, 16, 8, 8, vi, vw, vt, hi, hw, ht, st) == L.TG_E_ARG
    assert lib.tg_resample_u8(xd.data_ptr(), None, 1, 16, 16, 8, 8, vi, vw, vt, hi, hw, ht, st) == L.TG_E_ARG
    torch.cuda.synchronize()
    assert bool((y == GUARD).all())
    for bad in (xd.cpu(), xd.float(), xd.permute(0, 3, 1, 2), xd[0, :, :, 0]):
        with pytest.raises(L.TecoganHipError):
            ops.resize_u8(bad, (8, 8))
    for size in ((3, 8), (8, 65), (8,), 8, (0, 8)):
        with pytest.raises(L.TecoganHipError):
            ops.resize_u8(xd, size)
    with pytest.raises(L.TecoganHipError):
        ops.resize_u8(xd, (8, 8), out=torch.empty(1, 8, 9, 3, dtype=torch.uint8, device=DEV))


def test_a_wrong_table_stays_inside_the_frame():
    """Indices far outside [0, n_in - 1] and a footprint wider than a tile can stage: the indices are clamped, the call
    succeeds, the guards stay; a table whose every index is out of range reads the edge pixel."""
    x = np.random.RandomState(3).randint(0, 256, (1, 16, 16, 3)).astype(np.uint8)
    idx, w = ops.resample_tables(16, 8)
    far = torch.from_numpy(np.where(idx > 7, idx + 10 ** 6, idx - 10 ** 6).astype(np.int32)).to(DEV)
    wd = torch.from_numpy(w).to(DEV)
    t = (far.data_ptr(), wd.data_ptr(), idx.shape[1])
    rc, got, intact = _raw(x, 8, 8, 1, 1, tables=(t, t))
    assert rc == L.TG_OK and intact
    edge = np.where(idx > 7, 15, 0)
    want = R.round_sums(np.einsum('ok,pl,opklc->opc', w.astype(np.int64), w.astype(np.int64),
                                  x[0].astype(np.int64)[edge[:, None, :, None], edge[None, :, None, :]]))
    assert np.array_equal(got[0], want)
    # 300 x 300 -> 80 x 80 with the rows' indices alternating between the two ends of the frame: the footprint is the
    # whole frame, more than a tile stages
    xb = np.random.RandomState(4).randint(0, 256, (1, 300, 300, 3)).astype(np.uint8)
    idx, w = ops.resample_tables(300, 80)
    wide = idx.copy()
    wide[:, ::2] = 0
    wide[:, 1::2] = 299
    wide, wd = torch.from_numpy(wide).to(DEV), torch.from_numpy(w).to(DEV)
    t = (wide.data_ptr(), wd.data_ptr(), idx.shape[1])
    rc, got, intact = _raw(xb, 80, 80, 1, 1, tables=(t, t))
    assert rc == L.TG_OK and intact


# ------------------------------------------------------------------ the stream
def make_net(deg, s):
    from tecogan_pytorch_amd.models.networks import FRNet
    net = FRNet(3, 3, 64, 10, deg, s)
    net.load_state_dict(generator_state_dict(scale=s, degradation=deg), strict=True)
    return net.cuda().eval()


@pytest.fixture(scope='module')
def net4():
    return make_net('BD', 4)


H, W, SIZE = 16, 24, (36, 54)
CFG = ('bt709', False, 'left')
_CLIPS = {}


def _clip(t):
    """Per length, once: the I420 clip and the LR frames the yuv stream makes of it (fp32, on the host)."""
    if t not in _CLIPS:
        u8 = (smooth_clip(t, 3, H, W, seed=60 + t).permute(0, 2, 3, 1) * 255.0).round().clamp(0, 255).to(torch.uint8)
        i420 = np.ascontiguousarray(Y.rgb_to_yuv420(u8.numpy(), *CFG))
        lr = ops.yuv420_to_rgb(torch.from_numpy(i420).to(DEV), H, W, *CFG).cpu()
        _CLIPS[t] = (i420, lr)
    return _CLIPS[t]


def _chunkings(clip):
    t, uneven, pos, sizes = clip.shape[0], [], 0, [2, 5, 1, 11, 3, 7]
    while pos < t:
        m = min(t - pos, sizes[len(uneven) % len(sizes)])
        uneven.append(clip[pos:pos + m])
        pos += m
    return {'frames': [f for f in clip], 'uneven': uneven}


def _decode(png):
    with Image.open(io.BytesIO(bytes(png))) as im:
        assert im.mode == 'RGB'
        return np.asarray(im).copy()


@pytest.mark.parametrize('t', [1, 10])
def test_stream_yields_the_specification_of_the_frames_it_yields_without_resize(net4, t):
    from tecogan_pytorch_amd.models.networks import Png, Resize, Yuv420
    i420, lr = _clip(t)
    plain = np.concatenate([c.copy() for c in net4.infer_stream(iter([lr]), DEV)], 0)
    assert plain.shape == (t, 4 * H, 4 * W, 3)
    want = R.resize_u8(plain, *SIZE)
    want_yuv = Y.rgb_to_yuv420(want, *CFG)
    want_png = [P.encode(f, 'adaptive') for f in want]
    rs, spec = Resize(*SIZE), Yuv420(H, W, *CFG)
    for name, items in _chunkings(lr).items():
        chunks = [c.copy() for c in net4.infer_stream(iter(items), DEV, resize=rs)]
        assert all(c.dtype == np.uint8 and c.shape[1:] == SIZE + (3,) for c in chunks)
        got = np.concatenate(chunks, 0)
        assert got.shape == want.shape and np.array_equal(got, want), (name, int((got != want).sum()))
        files = [v.tobytes() for c in net4.infer_stream(iter(items), DEV, resize=rs, png=Png()) for v in c]
        assert len(files) == t
        for k in range(t):
            assert files[k] == want_png[k], (name, k)
            assert np.array_equal(_decode(files[k]), want[k]), (name, k)
    for name, items in _chunkings(i420).items():
        got = np.concatenate([c.copy() for c in net4.infer_stream(iter(items), DEV, yuv=spec, resize=rs)], 0)
        assert got.shape == want_yuv.shape == (t, SIZE[0] * SIZE[1] * 3 // 2)
        assert np.array_equal(got, want_yuv), (name, int((got != want_yuv).sum()))
    net4.check_faults()


def test_stream_resize_composes_with_scene_cut(net4):
    from tecogan_pytorch_amd.models.networks import Resize, SceneCut
    _, lr = _clip(10)
    sc = SceneCut(detect=False, at=[4])
    plain = np.concatenate([c.copy() for c in net4.infer_stream(iter([lr]), DEV, scene_cut=sc)], 0)
    assert sc.cuts == [4]
    got = np.concatenate([c.copy() for c in net4.infer_stream(iter([lr]), DEV, scene_cut=sc, resize=Resize(*SIZE))], 0)
    assert sc.cuts == [4] and np.array_equal(got, R.resize_u8(plain, *SIZE))
    with pytest.raises(ValueError, match='ratio'):                      # refused at the first item; the network stays usable
        list(net4.infer_stream(iter([lr]), DEV, resize=Resize(15, 54)))
    assert sum(len(c) for c in net4.infer_stream(iter([lr]), DEV, resize=Resize(*SIZE))) == 10


def test_cli_y4m_with_output_size(tmp_path):
    """One y4m -> y4m run with --output-size 48x36 (the shape changes: 96x64 is 3:2, 48x36 is 4:3): the header carries
    the new size and the A tag that keeps the display aspect, the frames are the API's."""
    import yaml
    from tecogan_pytorch_amd import main as M
    from tecogan_pytorch_amd.data.y4m import Y4MReader
    from tecogan_pytorch_amd.models import define_model
    from tecogan_pytorch_amd.models.networks import Resize, Yuv420
    pth = str(tmp_path / 'G_iter7.pth')
    torch.save(generator_state_dict(scale=4, degradation='BD'), pth)
    opt = M.default_opt()
    opt['model']['generator']['load_path'] = pth
    yml = str(tmp_path / 'infer.yml')
    with open(yml, 'w') as f:
        yaml.safe_dump(opt, f)
    t = 10
    i420, _ = _clip(t)
    src, dst = str(tmp_path / 'in.y4m'), str(tmp_path / 'out.y4m')
    with open(src, 'wb') as f:
        f.write(b'YUV4MPEG2 W24 H16 F25:1 Ip A1:1 C420mpeg2 XCOLORRANGE=LIMITED\n')
        for fr in i420:
            f.write(b'FRAME\n' + fr.tobytes())
    M.main(['--mode', 'infer', '--opt', yml, '--input', src, '--output', dst, '--output-size', '48x36'])
    rd = Y4MReader(io.BytesIO(open(dst, 'rb').read()))
    assert (rd.w, rd.h, rd.siting, rd.full_range) == (48, 36, 'left', False)
    assert rd.header['tags'] == ['F25:1', 'A9:8', 'C420mpeg2', 'XCOLORRANGE=LIMITED']      # 96 * 36 : 64 * 48
    got = np.stack([fr.copy() for fr in rd])
    ref_opt = M.default_opt()
    ref_opt.update({'is_train': False, 'dist': False, 'device': 'cuda', 'rank': 0, 'world_size': 1})
    ref_opt['model']['generator']['load_path'] = pth
    model = define_model(ref_opt)
    spec = Yuv420(H, W, *CFG)
    plain = np.concatenate([c.copy() for c in model.infer_stream(iter([f for f in i420]), yuv=spec)], 0)
    api = np.concatenate([c.copy() for c in model.infer_stream(iter([f for f in i420]), yuv=spec, resize=Resize(36, 48))], 0)
    assert plain.shape == (t, 64 * 96 * 3 // 2)
    assert got.shape == api.shape == (t, 36 * 48 * 3 // 2) and np.array_equal(got, api)


def test_cli_png_folder_with_output_size_both_encoders(tmp_path):
    """--output-size on the PNG-folder form: both encoders write the frames the API yields with Resize, 54x36."""
    import yaml
    from tecogan_pytorch_amd import main as M
    from tecogan_pytorch_amd.models import define_model
    from tecogan_pytorch_amd.models.networks import Resize
    pth = str(tmp_path / 'G_iter7.pth')
    torch.save(generator_state_dict(scale=4, degradation='BD'), pth)
    opt = M.default_opt()
    opt['model']['generator']['load_path'] = pth
    yml = str(tmp_path / 'infer.yml')
    with open(yml, 'w') as f:
        yaml.safe_dump(opt, f)
    t, src = 7, str(tmp_path / 'lr')
    u8 = (smooth_clip(t, 3, H, W, seed=9).permute(0, 2, 3, 1) * 255.0).round().clamp(0, 255).to(torch.uint8).contiguous()
    os.makedirs(src)
    for i in range(t):
        Image.fromarray(u8[i].numpy()).save(os.path.join(src, '%04d.png' % i))
    ref_opt = M.default_opt()
    ref_opt.update({'is_train': False, 'dist': False, 'device': 'cuda', 'rank': 0, 'world_size': 1})
    ref_opt['model']['generator']['load_path'] = pth
    model = define_model(ref_opt)
    api = np.concatenate([c.copy() for c in model.infer_stream(iter([f for f in u8.numpy()]), resize=Resize(*SIZE))], 0)
    assert api.shape == (t,) + SIZE + (3,)
    for enc in ('pillow', 'device'):
        dst = str(tmp_path / enc)
        M.main(['--mode', 'infer', '--opt', yml, '--input', src, '--output', dst, '--png-encoder', enc,
                '--output-size', '%dx%d' % (SIZE[1], SIZE[0])])
        names = sorted(os.listdir(dst))
        assert names == ['%04d.png' % i for i in range(t)]
        for k, n in enumerate(names):
            data = open(os.path.join(dst, n), 'rb').read()
            assert np.array_equal(_decode(data), api[k]), (enc, k)
            if enc == 'device':
                assert data == P.encode(api[k], 'adaptive'), k
