"""The device PNG encoder on the GPU: tg_png_encode_u8 equals tests/png_ref.py BYTE FOR BYTE on
every branch of the format, at every placement of `out` the ABI admits and without touching a byte outside its
regions; bad arguments are refused without a launch; FRNet.infer_stream(png=...) yields the files of the frames the
stream yields without it, through a repair as well; `--mode infer --png-encoder device` writes the pixels that
`--png-encoder pillow` writes."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

from procedural_weights import generator_state_dict, smooth_clip
from tests import png_ref as P

ROOT_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_DIR = os.path.join(ROOT_DIR, 'tests', 'golden')
DEV = torch.device('cuda', 0)
CASES = P.cases()
_REF = {}


def ref(img, filter):
    """png_ref.encode, computed once per frame and filter."""
    key = (img.shape, img.tobytes(), filter)
    if key not in _REF:
        _REF[key] = P.encode(img, filter)
    return _REF[key]


def neighbours(img):
    """Two frames of img's size and of other kinds: noise (stored segments) and a constant (a tree of two)."""
    rs = np.random.RandomState(img.shape[0] * 7 + img.shape[1])
    return [rs.randint(0, 256, img.shape).astype(np.uint8), np.full(img.shape, 131, np.uint8)]


def decode(png):
    with Image.open(io.BytesIO(bytes(png))) as im:
        assert im.mode == 'RGB'
        return np.asarray(im).copy()


# ------------------------------------------------------------------ ops.png_encode against the specification
@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('filter', P.FILTERS)
@pytest.mark.parametrize('name,img', CASES, ids=[c[0] for c in CASES])
def test_png_encode_equals_the_specification_byte_for_byte(name, img, filter, n):
    from tecogan_pytorch_amd import ops
    # (with n = 3 frames of different kinds share one launch: a frame's bytes cannot depend on its neighbours)
    frames = [img] if n == 1 else [neighbours(img)[0], img, neighbours(img)[1]]
    x = torch.from_numpy(np.stack(frames)).to(DEV)
    got = ops.png_encode(x if n > 1 else x[0], filter)
    assert len(got) == n
    for k, frame in enumerate(frames):
        want = ref(frame, filter)
        assert len(got[k]) == len(want), (name, filter, k, len(got[k]), len(want))
        assert got[k] == want, (name, filter, k, next(i for i in range(len(want)) if got[k][i] != want[i]))
    assert np.array_equal(decode(got[n // 2]), img)


def test_more_segments_than_threads_per_workgroup():
    """259 segments: the offset sums, the Adler-32 and the CRC-32 are combined across more segments than a workgroup
    has threads.  The specification in numpy would take seconds at this size; zlib checks the Adler-32 and Pillow the
    CRCs when they decode, and the IDAT must be the filtered stream."""
    import zlib
    from tecogan_pytorch_amd import ops
    h, w = 300, 9400
    assert -(-h * (3 * w + 1) // P.SEG) == 259
    y, x = np.mgrid[0:h, 0:w]
    img = np.stack([(x // 5 + y) % 256, (x // 3 + 2 * y) % 256, (x // 7) % 256], axis=2).astype(np.uint8)
    img[100:200] = np.random.RandomState(5).randint(0, 256, (100, w, 3))          # stored segments in the middle
    png, = ops.png_encode(torch.from_numpy(img).to(DEV), 'none')
    assert len(png) <= P.capacity(h, w)
    chunks = P.chunks(png)
    assert [c[0] for c in chunks] == [b'IHDR', b'IDAT', b'IEND']
    assert all(crc == zlib.crc32(kind + data) for kind, data, crc in chunks)
    rows = np.concatenate([np.zeros((h, 1), np.uint8), img.reshape(h, 3 * w)], axis=1)   # type 0 on every row
    assert zlib.decompress(chunks[1][1]) == rows.tobytes()
    assert np.array_equal(decode(png), img)


def _raw_encode(frames, filter, offset, extra_stride, guard=64):
    """tg_png_encode_u8 with `out` `offset` bytes into its allocation, a stride of capacity + extra_stride, and
    `guard` bytes of 0xA5 before `out` and behind out + n * stride.  -> (files, sizes, the whole allocation)."""
    from tecogan_pytorch_amd import _lib as L
    lib = L.lib()
    n, h, w = len(frames), frames[0].shape[0], frames[0].shape[1]
    x = torch.from_numpy(np.stack(frames)).to(DEV)
    cap = lib.tg_png_capacity(h, w)
    assert cap == P.capacity(h, w)
    stride = cap + extra_stride
    buf = torch.full((guard + offset + n * stride + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    sizes = torch.zeros(n, dtype=torch.int64, device=DEV)
    ws = torch.empty(lib.tg_png_workspace_bytes(n, h, w), dtype=torch.uint8, device=DEV)
    out = buf.data_ptr() + guard + offset
    L.check(lib.tg_png_encode_u8(x.data_ptr(), n, h, w, L.PNG_FILTER[filter], out, stride, sizes.data_ptr(),
                                 ws.data_ptr(), torch.cuda.current_stream().cuda_stream), 'tg_png_encode_u8')
    torch.cuda.synchronize()
    host, sizes = buf.cpu().numpy(), sizes.cpu().tolist()
    files = [host[guard + offset + k * stride:guard + offset + k * stride + sizes[k]].tobytes() for k in range(n)]
    return files, sizes, host, guard + offset, stride


@pytest.mark.parametrize('offset,extra', [(0, 0), (1, 13), (3, 1), (1, 0)])
def test_out_at_any_offset_and_stride_and_nothing_outside_is_written(offset, extra):
    img = dict(CASES)['64x176 smooth']
    frames = [img] + neighbours(img)
    files, sizes, host, first, stride = _raw_encode(frames, 'adaptive', offset, extra)
    for k, frame in enumerate(frames):
        assert sizes[k] == len(ref(frame, 'adaptive')) and files[k] == ref(frame, 'adaptive'), (offset, extra, k)
    assert (host[:first] == 0xA5).all() and (host[first + 3 * stride:] == 0xA5).all()
    assert host[first + 3 * stride:].size == 64


def test_bad_arguments_are_refused_without_a_launch():
    from tecogan_pytorch_amd import _lib as L
    lib = L.lib()
    h, w = 8, 8
    x = torch.zeros(2, h, w, 3, dtype=torch.uint8, device=DEV)
    cap = lib.tg_png_capacity(h, w)
    out = torch.full((2 * cap,), 0xA5, dtype=torch.uint8, device=DEV)
    sizes = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    ws = torch.empty(lib.tg_png_workspace_bytes(2, h, w), dtype=torch.uint8, device=DEV)
    good = dict(rgb=x.data_ptr(), n=2, h=h, w=w, filter=1, out=out.data_ptr(), stride=cap, sizes=sizes.data_ptr(),
                ws=ws.data_ptr())
    bad = [(dict(rgb=None), L.TG_E_ARG, 'null'), (dict(out=None), L.TG_E_ARG, 'null'),
           (dict(sizes=None), L.TG_E_ARG, 'null'), (dict(ws=None), L.TG_E_ARG, 'null'),
           (dict(h=0), L.TG_E_ARG, 'h=0'), (dict(w=0), L.TG_E_ARG, 'w=0'), (dict(w=-3), L.TG_E_ARG, 'w=-3'),
           (dict(n=0), L.TG_E_ARG, 'n=0'), (dict(filter=2), L.TG_E_ARG, 'filter=2'),
           (dict(h=1 << 16, w=1 << 14, stride=1 << 40), L.TG_E_SHAPE, '2^31'),
           (dict(stride=cap - 1), L.TG_E_SHAPE, 'out_stride=%d' % (cap - 1))]
    for change, code, word in bad:
        a = dict(good, **change)
        rc = lib.tg_png_encode_u8(a['rgb'], a['n'], a['h'], a['w'], a['filter'], a['out'], a['stride'], a['sizes'],
                                  a['ws'], torch.cuda.current_stream().cuda_stream)
        msg = lib.tg_last_error_string().decode()
        assert rc == code and 'png_encode_u8' in msg and word in msg, (change, rc, msg)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0xA5).all() and sizes.cpu().tolist() == [-7, -7]          # nothing ran
    assert lib.tg_png_capacity(0, 8) == -1 and lib.tg_png_capacity(1 << 16, 1 << 14) == -1
    assert lib.tg_png_workspace_bytes(0, 8, 8) == -1 and lib.tg_png_workspace_bytes(1, 8, 0) == -1
    assert lib.tg_png_capacity(1, 1) == 72 and lib.tg_png_capacity(129, 85) == P.capacity(129, 85)
    from tecogan_pytorch_amd import ops
    for args in ((x.cpu(),), (x.float(),), (x[..., :2],), (x, 'paeth')):
        with pytest.raises(L.TecoganHipError):
            ops.png_encode(*args)


# ------------------------------------------------------------------ the stream
def make_net(deg, s):
    from tecogan_pytorch_amd.models.networks import FRNet
    net = FRNet(3, 3, 64, 10, deg, s)
    net.load_state_dict(generator_state_dict(scale=s, degradation=deg), strict=True)
    return net.cuda().eval()


def files_of(net, items, **kw):
    """The whole png stream, every view copied out of its ring slot: [bytes]."""
    from tecogan_pytorch_amd.models.networks import Png
    out = []
    for chunk in net.infer_stream(iter(items), DEV, png=kw.pop('png', Png()), **kw):
        assert isinstance(chunk, list) and all(v.dtype == np.uint8 and v.ndim == 1 for v in chunk)
        out.extend(v.tobytes() for v in chunk)
    return out


def uneven(clip):
    parts, pos, sizes = [], 0, [2, 5, 1, 11, 3, 7]
    while pos < clip.shape[0]:
        parts.append(clip[pos:pos + sizes[len(parts) % len(sizes)]])
        pos += parts[-1].shape[0]
    return parts


@pytest.fixture(scope='module')
def net2():
    return make_net('BI', 2)


@pytest.mark.parametrize('t', [1, 10, 30])
def test_stream_yields_the_files_of_the_frames_it_yields_without_png(net2, t):
    from tecogan_pytorch_amd import ops
    from tecogan_pytorch_amd.models.networks import Png
    clip = smooth_clip(t, 3, 16, 24, seed=40 + t)
    rgb = np.concatenate([c.copy() for c in net2.infer_stream(iter([clip]), DEV)], 0)
    assert rgb.shape == (t, 32, 48, 3)
    want = ops.png_encode(torch.from_numpy(rgb).to(DEV))
    assert want[0] == ref(rgb[0], 'adaptive') and want[-1] == ref(rgb[-1], 'adaptive')
    for items in ([f for f in clip], uneven(clip)):
        got = files_of(net2, items)
        assert len(got) == t
        for k in range(t):
            assert np.array_equal(decode(got[k]), rgb[k]), (t, k)
            assert got[k] == want[k], (t, k)
    none = files_of(net2, [clip], png=Png('none'))
    assert none == ops.png_encode(torch.from_numpy(rgb).to(DEV), 'none')


def test_stream_full_size_on_the_resident_launch():
    import ctypes
    from tecogan_pytorch_amd import _lib, ops
    net = make_net('BD', 4)
    clip = smooth_clip(10, 3, 134, 320, seed=3)
    rgb = np.concatenate([c.copy() for c in net.infer_stream(iter([clip]), DEV)], 0)
    got = files_of(net, uneven(clip))
    assert len(got) == 10 and got == ops.png_encode(torch.from_numpy(rgb).to(DEV))
    assert got[4] == ref(rgb[4], 'adaptive')                     # 63 segments
    for k in range(10):
        assert np.array_equal(decode(got[k]), rgb[k]), k
    lib = _lib.lib()
    plan = net._get_plan(1, 134, 320, DEV)
    names = [lib.tg_frnet_kind_name(k).decode() for k in range(lib.tg_frnet_plan_kinds())]
    nl = ctypes.c_int()
    _lib.check(lib.tg_frnet_plan_kind_stats(plan.handle, names.index('conv3x3_wino_resident_kernel'), ctypes.byref(nl),
                                            None, None), 'kind_stats')
    assert nl.value == 1 and plan.chain_state() == (0, True)


def test_vsr_model_stream_drops_the_padded_prefix():
    from tecogan_pytorch_amd.main import default_opt
    from tecogan_pytorch_amd.models import define_model
    from tecogan_pytorch_amd.models.networks import Png
    opt = default_opt()
    opt.update({'is_train': False, 'dist': False, 'device': 'cuda', 'rank': 0, 'world_size': 1})
    model = define_model(opt)
    model.net_G.load_state_dict(generator_state_dict(scale=4, degradation='BD'), strict=True)
    clip = smooth_clip(13, 3, 24, 40, seed=6)
    rgb = np.concatenate([c.copy() for c in model.infer_stream(f for f in clip)], 0)
    got = [v.tobytes() for chunk in model.infer_stream((f for f in clip), png=Png()) for v in chunk]
    assert len(got) == 13 and all(np.array_equal(decode(g), f) for g, f in zip(got, rgb))


# ------------------------------------------------------------------ a repaired batch is encoded again
_REPAIR = (
    "import sys, torch, warnings; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
    "import numpy as np\n"
    "from tests.test_hip_png import make_net, files_of, DEV\n"
    "from procedural_weights import smooth_clip\n"
    "from tecogan_pytorch_amd import _lib\n"
    "from tecogan_pytorch_amd.models.networks import Png\n"
    "H, W = 40, 72\n"
    "limit = lambda plan, v: _lib.check(_lib.lib().tg_frnet_plan_set_chain_poll_limit(plan.handle, v), 'limit')\n"
    "clip = smooth_clip(40, 3, H, W, seed=5)\n"
    "net = make_net('BD', 4); plan = net._get_plan(1, H, W, DEV)\n"
    "assert plan.chain_state() == (0, True), plan.chain_state()\n"
    "clean = files_of(net, [f for f in clip])\n"
    "assert plan.chain_state() == (0, True)\n"
    "net = make_net('BD', 4); plan = net._get_plan(1, H, W, DEV)\n"
    "out = []\n"
    "with warnings.catch_warnings(record=True) as wl:\n"
    "    warnings.simplefilter('always')\n"
    "    gen = net.infer_stream(iter([f for f in clip]), DEV, png=Png())\n"
    "    out.extend(v.tobytes() for v in next(gen))\n"
    "    limit(plan, -1)                       # the project's time-out injection (tests/test_hip_stream.py)\n"
    "    out.extend(v.tobytes() for v in next(gen))\n"
    "    limit(plan, 1 << 21)\n"
    "    for chunk in gen: out.extend(v.tobytes() for v in chunk)\n"
    "msgs = [str(w_.message) for w_ in wl if issubclass(w_.category, RuntimeWarning)]\n"
    "assert len(msgs) == 1 and 'computed again' in msgs[0], msgs\n"
    "f, active = plan.chain_state(); assert f > 0 and not active, (f, active)\n"
    "assert len(out) == 40 and out == clean, 'repaired stream differs'\n"
    "print('PNG-REPAIR-OK')\n" % (ROOT_DIR, GOLDEN_DIR))


def test_a_repaired_stream_yields_the_same_files():
    env = dict(os.environ, TG_WINO_RES='1', TG_CONV_WINO='1', TG_WINO_RES_CT='0')       # as tests/test_hip_stream.py
    r = subprocess.run([sys.executable, '-c', _REPAIR], env=env, timeout=600, capture_output=True, text=True)
    assert r.returncode == 0 and 'PNG-REPAIR-OK' in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# ------------------------------------------------------------------ the CLI
def test_cli_device_encoder_writes_the_pixels_of_the_pillow_encoder(tmp_path):
    import yaml
    from tecogan_pytorch_amd import main as M
    pth = str(tmp_path / 'G_iter7.pth')
    torch.save(generator_state_dict(scale=4, degradation='BD'), pth)
    opt = M.default_opt()
    opt['model']['generator']['load_path'] = pth
    yml = str(tmp_path / 'infer.yml')
    with open(yml, 'w') as f:
        yaml.safe_dump(opt, f)
    src = str(tmp_path / 'lr')
    clip = smooth_clip(12, 3, 24, 40, seed=9)
    u8 = (clip.permute(0, 2, 3, 1) * 255.0).round().clamp(0, 255).to(torch.uint8).contiguous()
    os.makedirs(os.path.join(src, 'walk'))
    for i in range(12):
        Image.fromarray(u8[i].numpy()).save(os.path.join(src, 'walk', '%04d.png' % i))
    out = {}
    for enc in ('pillow', 'device'):
        dst = str(tmp_path / enc)
        M.main(['--mode', 'infer', '--opt', yml, '--input', src, '--output', dst, '--png-encoder', enc])
        names = sorted(os.listdir(os.path.join(dst, 'walk')))
        assert names == ['%04d.png' % i for i in range(12)]
        out[enc] = [open(os.path.join(dst, 'walk', n), 'rb').read() for n in names]
    for k in range(12):
        a, b = decode(out['pillow'][k]), decode(out['device'][k])
        assert a.shape == (96, 160, 3) and np.array_equal(a, b), k
        assert out['device'][k] == ref(a, 'adaptive'), k        # the file is the specification's
