"""Motion-adaptive deinterlacing on the GPU: tg_deinterlace_planar through the C ABI against
tests/deinterlace_ref.py, sample for sample with no tolerance -- three layouts, 8 / 10 / 12 bits, both field orders, with
and without a frame before, every field window of a 3-frame clip, at the smallest shapes that reach the element form,
the 16-byte form, partial pieces and an off-alignment placement, with guard bytes around the output and behind the
input; the error contract; ops.deinterlace; FRNet.infer_stream(yuv=..., deinterlace=...) against the SAME stream without
the option fed the specification's progressive frames; and --mode infer on an interlaced y4m clip."""
import io

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from procedural_weights import generator_state_dict
from tests import deinterlace_ref as R
from tests.test_hip_yuv_depth import make_net

DEV = torch.device('cuda', 0)
GUARD = 0xA5
PAD = 64
E_ARG = -2
K = 3
# (first_field, step, cnt) on K = 3 frames: the window ends on either parity, at both rates
WINDOWS = [(0, 1, 6), (0, 1, 5), (1, 1, 4), (1, 1, 5), (0, 2, 3), (1, 2, 3), (1, 2, 2)]
# the smallest shapes that reach each path (h, w): every row a border row and every column clamped; no 16-byte piece and
# an odd chroma width; the wide form, an exact multiple; a wide body with a partial piece behind it
SHAPES = [(4, 2), (8, 18), (8, 64), (12, 70)]
CASES = [(c, d, h, w) for c in ('420', '422', '444') for d in (8, 10) for (h, w) in SHAPES] + \
    [('422', 8, 12, 50), ('422', 10, 12, 50), ('420', 12, 8, 64), ('444', 12, 8, 18)]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def gpu_deinterlace(run, h, w, chroma, depth, tff, has_prev, first_field, step, cnt, off=0, expect=0):
    """tg_deinterlace_planar on `run` ((k + 1, samples) numpy: the frame before, then the k frames) -> (cnt, samples)
    numpy.  Both buffers start PAD + off bytes into a 256-byte aligned allocation; the bytes before and behind the
    output and behind the input are guards and must stay."""
    from tecogan_pytorch_amd import _lib as L
    raw = torch.from_numpy(np.ascontiguousarray(run).view(np.uint8).reshape(-1))
    src = torch.full((PAD + off + raw.numel() + PAD,), GUARD, dtype=torch.uint8, device=DEV)
    src[PAD + off:PAD + off + raw.numel()].copy_(raw)
    nbytes = cnt * run.shape[1] * run.dtype.itemsize
    dst = torch.full((PAD + off + nbytes + PAD,), GUARD, dtype=torch.uint8, device=DEV)
    assert src.data_ptr() % 256 == 0 and dst.data_ptr() % 256 == 0
    rc = L.lib().tg_deinterlace_planar(src.data_ptr() + PAD + off, dst.data_ptr() + PAD + off, run.shape[0] - 1, h, w,
                                       L.YUV_CHROMA[chroma], depth, tff, has_prev, first_field, step, cnt, _stream())
    torch.cuda.synchronize()
    assert rc == expect, (rc, L.lib().tg_last_error_string())
    host = dst.cpu().numpy()
    assert (host[:PAD + off] == GUARD).all() and (host[PAD + off + nbytes:] == GUARD).all(), 'wrote outside its output'
    assert bool((src[PAD + off + raw.numel():] == GUARD).all()) and bool((src[:PAD + off] == GUARD).all())
    return host[PAD + off:PAD + off + nbytes].view(run.dtype).reshape(cnt, run.shape[1])


def clips(h, w, chroma, depth, seed):
    """{name: (K + 1, samples)}: noise (16-bit: a few words above the depth's maximum), a static picture, and a smooth
    picture that moves one column per frame."""
    rng = np.random.default_rng(seed)
    ns, top = R.frame_samples(h, w, chroma), (1 << depth) - 1
    dt = np.uint8 if depth == 8 else np.uint16
    noise = rng.integers(0, top + 1, (K + 1, ns)).astype(dt)
    if depth > 8:
        noise[:, ::7] = 65535
    static = np.repeat(rng.integers(0, top + 1, (1, ns)).astype(dt), K + 1, 0)
    moving = np.empty((K + 1, ns), dt)
    for t in range(K + 1):
        planes = []
        for ph, pw in R.plane_shapes(h, w, chroma):
            y, x = np.mgrid[0:ph, 0:pw]
            planes.append(((np.sin(0.9 * (x - t) + 0.7 * y) * 0.5 + 0.5) * top).round().astype(dt).reshape(-1))
        moving[t] = np.concatenate(planes)
    return {'noise': noise, 'static': static, 'moving': moving}


def spec_of(run, h, w, chroma, depth, tff, has_prev, first_field, step, cnt, stats=None):
    return R.deinterlace(run[1:], h, w, chroma, depth, bool(tff), run[0] if has_prev else None, first_field, step, cnt, stats)


@pytest.mark.parametrize('chroma,depth,h,w', CASES)
def test_kernel_equals_the_specification_sample_for_sample(chroma, depth, h, w):
    stats = {}
    for name, run in clips(h, w, chroma, depth, 7 + h + w).items():
        for tff in (0, 1):
            for has_prev in (0, 1):
                for (ff, step, cnt) in (WINDOWS if name == 'noise' else WINDOWS[:1]):
                    src = run.copy()
                    if not has_prev:
                        src[0] = 0x5A if depth == 8 else 0x5A5A            # never read: any content gives the same result
                    got = gpu_deinterlace(src, h, w, chroma, depth, tff, has_prev, ff, step, cnt)
                    ref = spec_of(run, h, w, chroma, depth, tff, has_prev, ff, step, cnt, stats)
                    assert np.array_equal(got, ref), (name, tff, has_prev, ff, step, cnt, int((got != ref).sum()))
    # the inputs reach every branch of the specification: each direction wins somewhere, both motion bounds clamp
    assert all(stats.get(('dir', d), 0) > 0 for d in R.DIRECTIONS), stats
    assert stats.get('lo', 0) > 0 and stats.get('hi', 0) > 0 and 0 < stats['sp'] < stats['n'], stats


@pytest.mark.parametrize('depth', [8, 10])
@pytest.mark.parametrize('chroma', ['420', '444'])
def test_a_base_off_its_alignment_takes_the_element_form_and_gives_the_same_samples(chroma, depth):
    h, w = 8, 64
    run = clips(h, w, chroma, depth, 3)['noise']
    off = 1 if depth == 8 else 16 + 2                       # one sample; for the words 16 bytes and one sample
    for tff, has_prev, (ff, step, cnt) in [(1, 1, WINDOWS[0]), (0, 0, WINDOWS[3]), (1, 1, WINDOWS[5])]:
        a = gpu_deinterlace(run, h, w, chroma, depth, tff, has_prev, ff, step, cnt)
        b = gpu_deinterlace(run, h, w, chroma, depth, tff, has_prev, ff, step, cnt, off=off)
        assert np.array_equal(a, b) and np.array_equal(a, spec_of(run, h, w, chroma, depth, tff, has_prev, ff, step, cnt))


def test_every_refusal_is_tg_e_arg_without_a_launch():
    from tecogan_pytorch_amd import _lib as L
    h, w = 8, 16
    run = clips(h, w, '420', 8, 1)['noise']
    ok = dict(h=h, w=w, chroma='420', depth=8, tff=1, has_prev=1, first_field=0, step=1, cnt=6)
    assert gpu_deinterlace(run, **ok).shape == (6, run.shape[1])
    bad = [dict(depth=9), dict(depth=16), dict(tff=2), dict(has_prev=-1), dict(first_field=2), dict(step=3), dict(step=0),
           dict(cnt=0), dict(cnt=7), dict(first_field=1, cnt=6), dict(step=2, cnt=4), dict(first_field=1, step=2, cnt=4),
           dict(h=6), dict(h=2), dict(w=1), dict(h=7)]
    for change in bad:
        out = gpu_deinterlace(run, **dict(ok, **change), expect=E_ARG)
        assert (out.view(np.uint8) == GUARD).all(), change
    # what the helper cannot express: null pointers, an unknown layout, k < 1, words at an odd address
    lib, st = L.lib(), _stream()
    buf = torch.full((4096,), GUARD, dtype=torch.uint8, device=DEV)
    src, dst = buf.data_ptr(), buf.data_ptr() + 2048
    for args in [(None, dst, 3, h, w, 0, 8, 1, 1, 0, 1, 6), (src, None, 3, h, w, 0, 8, 1, 1, 0, 1, 6),
                 (src, dst, 3, h, w, 3, 8, 1, 1, 0, 1, 6), (src, dst, 3, h, w, -1, 8, 1, 1, 0, 1, 6),
                 (src, dst, 0, h, w, 0, 8, 1, 1, 0, 1, 1), (src + 1, dst, 3, h, w, 0, 10, 1, 1, 0, 1, 2),
                 (src, dst + 1, 3, h, w, 0, 12, 1, 1, 0, 1, 2)]:
        assert lib.tg_deinterlace_planar(*args, st) == E_ARG, args
    torch.cuda.synchronize()
    assert bool((buf == GUARD).all())


def test_ops_deinterlace_with_and_without_prev_and_out():
    from tecogan_pytorch_amd import _lib as L, ops
    h, w = 8, 24
    for chroma, depth in (('420', 8), ('422', 10)):
        run = clips(h, w, chroma, depth, 5)['noise']
        dev = torch.from_numpy(run).to(DEV)
        cold = ops.deinterlace(dev[1:], h, w, chroma, depth)
        assert cold.shape == (2 * K, run.shape[1]) and cold.dtype == dev.dtype
        assert np.array_equal(cold.cpu().numpy(), R.deinterlace(run[1:], h, w, chroma, depth))
        out = torch.empty(K, run.shape[1], dtype=dev.dtype, device=DEV)
        got = ops.deinterlace(dev[1:], h, w, chroma, depth, tff=False, rate='frame', prev=dev[0], out=out)
        assert got is out
        assert np.array_equal(out.cpu().numpy(), R.deinterlace(run[1:], h, w, chroma, depth, False, run[0], 0, 2))
        warm = ops.deinterlace(dev[1:], h, w, chroma, depth, prev=dev[:1])
        assert np.array_equal(warm.cpu().numpy(), R.deinterlace(run[1:], h, w, chroma, depth, True, run[0]))
        assert not np.array_equal(warm[:2].cpu().numpy(), cold[:2].cpu().numpy())
    dev8 = torch.from_numpy(clips(h, w, '420', 8, 5)['noise']).to(DEV)
    for bad in (dict(rate='fields'), dict(chroma='411'), dict(depth=9), dict(out=torch.empty(1, 1, dtype=torch.uint8, device=DEV)),
                dict(prev=dev8[0, :5])):
        with pytest.raises(L.TecoganHipError):
            ops.deinterlace(dev8[1:], h, w, **bad)
    with pytest.raises(L.TecoganHipError):
        ops.deinterlace(dev8[1:].cpu(), h, w)


# ------------------------------------------------------------------ the stream
@pytest.fixture(scope='module')
def net4():
    return make_net('BD', 4)


def interlaced_clip(t, h, w, chroma, depth, seed):
    """(t, frame_bytes) uint8: the weave of a smooth picture that moves every FIELD, plus a little noise, top field first."""
    rng = np.random.default_rng(seed)
    top, dt = (1 << depth) - 1, np.uint8 if depth == 8 else np.uint16
    out = np.empty((t, R.frame_samples(h, w, chroma)), dt)
    for i in range(t):
        planes = []
        for ph, pw in R.plane_shapes(h, w, chroma):
            y, x = np.mgrid[0:ph, 0:pw]
            f = 2 * i + (y % 2)                                      # the field a row belongs to
            v = (np.sin(0.5 * (x - 0.8 * f) + 0.4 * y) * 0.4 + 0.5) * top + rng.integers(-3, 4, (ph, pw))
            planes.append(np.clip(v.round(), 0, top).astype(dt).reshape(-1))
        out[i] = np.concatenate(planes)
    return out.view(np.uint8)


def streamed(net, items, spec, ofb=None, **kw):
    out = [c.copy() for c in net.infer_stream(iter(items), DEV, yuv=spec, **kw)]
    ofb = spec.out_frame_bytes(net.scale) if ofb is None else ofb
    assert all(c.dtype == np.uint8 and c.ndim == 2 and c.shape[1] == ofb for c in out)
    return np.concatenate(out, 0) if out else np.zeros((0, ofb), np.uint8), [len(c) for c in out]


def progressive(clip, spec, deint):
    """The specification's progressive frames of the interlaced clip, as the bytes the stream takes."""
    samples = clip if spec.depth == 8 else clip.view(np.uint16)
    return np.ascontiguousarray(R.stream(samples, spec.h, spec.w, spec.chroma, spec.depth, deint.tff, deint.rate)).view(np.uint8)


def _specs():
    from tecogan_pytorch_amd.models.networks import Yuv, Yuv420
    return {'420': Yuv420(16, 24), '422p10': Yuv(16, 24, '422', '444', 'bt2020', False, 'left', depth=10)}


@pytest.fixture(scope='module')
def stream_refs(net4):
    """Per spec: the 11-frame interlaced clip, its progressive frames at field rate and what the stream WITHOUT the
    option yields for those; computed once and shared."""
    from tecogan_pytorch_amd.models.networks import Deinterlace
    refs = {}
    for name, spec in _specs().items():
        clip = interlaced_clip(11, 16, 24, spec.chroma, spec.depth, 21)
        prog = progressive(clip, spec, Deinterlace())
        ref, sizes = streamed(net4, [prog], spec)
        assert ref.shape[0] == 22 and sizes == [9, 8, 5]
        refs[name] = (spec, clip, prog, ref)
    return refs


@pytest.mark.parametrize('name', ['420', '422p10'])
def test_stream_equals_the_plain_stream_on_the_specifications_frames(net4, stream_refs, name):
    from tecogan_pytorch_amd.models.networks import Deinterlace
    spec, clip, prog, ref = stream_refs[name]
    forms = {'frames': [f for f in clip], 'chunks': [clip[:3], clip[3:8], clip[8:]], 'whole': [clip]}
    if spec.depth > 8:
        forms['samples'] = [c.view(np.uint16) for c in forms['chunks']]
    for form, items in forms.items():
        got, sizes = streamed(net4, items, spec, deinterlace=Deinterlace())
        assert sizes == [9, 8, 5], form                     # (the frame at the first border has a field in each batch)
        assert got.shape == ref.shape and np.array_equal(got, ref), (form, int((got != ref).sum()))


@pytest.mark.parametrize('name', ['420', '422p10'])
def test_stream_at_frame_rate_bottom_field_first_and_a_one_frame_stream(net4, stream_refs, name):
    from tecogan_pytorch_amd.models.networks import Deinterlace
    spec, clip, _, ref_field = stream_refs[name]
    deint = Deinterlace(tff=False, rate='frame')
    got, sizes = streamed(net4, [clip[:4], clip[4:]], spec, deinterlace=deint)
    ref, _ = streamed(net4, [progressive(clip, spec, deint)], spec)
    assert sizes == [9, 2] and np.array_equal(got, ref) and not np.array_equal(got, ref_field[::2])
    for d in (Deinterlace(), Deinterlace(rate='frame')):
        one, sizes = streamed(net4, [clip[0]], spec, deinterlace=d)
        assert sizes == [d.per_frame]
        assert np.array_equal(one, streamed(net4, [progressive(clip[:1], spec, d)], spec)[0])
    assert streamed(net4, [], spec, deinterlace=Deinterlace())[0].shape[0] == 0


def test_stream_with_a_forced_scene_cut_in_output_numbering(net4, stream_refs):
    from tecogan_pytorch_amd.models.networks import Deinterlace, SceneCut
    spec, clip, prog, ref = stream_refs['420']
    sc = SceneCut(detect=False, at=(9,))
    got, _ = streamed(net4, [f for f in clip], spec, deinterlace=Deinterlace(), scene_cut=sc)
    assert sc.cuts == [9]
    assert np.array_equal(got[:9], ref[:9]) and not np.array_equal(got[9:], ref[9:])
    assert np.array_equal(got[9:], streamed(net4, [prog[9:]], spec)[0])       # a clip of its own from output frame 9 on


def test_stream_with_a_resize(net4, stream_refs):
    from tecogan_pytorch_amd.models.networks import Deinterlace, Resize
    spec, clip, prog, _ = stream_refs['420']
    ofb = 48 * 72 * 3 // 2
    got, _ = streamed(net4, [clip[:5], clip[5:]], spec, ofb=ofb, deinterlace=Deinterlace(), resize=Resize(48, 72))
    ref, _ = streamed(net4, [prog], spec, ofb=ofb, resize=Resize(48, 72))
    assert got.shape == (22, ofb) and np.array_equal(got, ref)


def test_refusals_before_anything_is_pulled_or_allocated(net4):
    from tecogan_pytorch_amd.models.networks import Deinterlace, Yuv, Yuv420
    pulled = []

    def items():
        pulled.append(1)
        yield np.zeros(10, np.uint8)
    before = torch.cuda.memory_allocated(DEV)
    with pytest.raises(ValueError, match='yuv'):
        net4.infer_stream(items(), DEV, deinterlace=Deinterlace())
    with pytest.raises(ValueError, match='multiple of 4'):
        net4.infer_stream(items(), DEV, yuv=Yuv420(18, 24), deinterlace=Deinterlace())
    with pytest.raises(ValueError, match='multiple of 2'):
        net4.infer_stream(items(), DEV, yuv=Yuv(17, 24, '444'), deinterlace=Deinterlace())
    with pytest.raises(ValueError, match='Deinterlace'):
        net4.infer_stream(items(), DEV, yuv=Yuv420(16, 24), deinterlace='tff')
    assert pulled == [] and torch.cuda.memory_allocated(DEV) == before


# ------------------------------------------------------------------ --mode infer
def test_infer_y4m_on_an_interlaced_clip(tmp_path, net4):
    import yaml
    from tecogan_pytorch_amd import main as M
    from tecogan_pytorch_amd.data.y4m import Y4MError, Y4MReader
    from tecogan_pytorch_amd.models.networks import Deinterlace, Yuv420
    pth = str(tmp_path / 'G_iter7.pth')
    torch.save(generator_state_dict(scale=4, degradation='BD'), pth)
    opt = M.default_opt()
    opt['model']['generator']['load_path'] = pth
    opt.update({'is_train': False, 'dist': False, 'device': 'cuda', 'rank': 0, 'world_size': 1})      # (what main.setup adds)
    assert opt['test']['num_pad_front'] > 0                # skipped with deinterlace: the stream starts cold
    h, w, t = 16, 24, 5
    spec = Yuv420(h, w, 'bt709', False, 'left')
    clip = interlaced_clip(t, h, w, '420', 8, 9)
    data = b'YUV4MPEG2 W24 H16 F30000:1001 It A1:1 C420mpeg2\n' + b''.join(b'FRAME\n' + f.tobytes() for f in clip)
    dst = io.BytesIO()
    assert M.infer_y4m(opt, io.BytesIO(data), dst, deinterlace='auto') == 2 * t
    rd = Y4MReader(io.BytesIO(dst.getvalue()))              # (a default reader: the header written says Ip)
    assert (rd.w, rd.h, rd.interlace) == (96, 64, 'p') and rd.header['tags'] == ['F60000:1001', 'A1:1', 'C420mpeg2']
    got = np.stack([f.copy() for f in rd])
    ref, _ = streamed(net4, [clip], spec, deinterlace=Deinterlace(tff=True))
    assert got.shape == ref.shape == (2 * t, spec.out_frame_bytes(4)) and np.array_equal(got, ref)
    # forced bottom field first at the input's rate, on the same (mis-tagged) stream
    dst = io.BytesIO()
    assert M.infer_y4m(opt, io.BytesIO(data), dst, deinterlace='bff', deinterlace_rate='frame') == t
    rd = Y4MReader(io.BytesIO(dst.getvalue()))
    assert rd.header['tags'][0] == 'F30000:1001'
    ref, _ = streamed(net4, [clip], spec, deinterlace=Deinterlace(tff=False, rate='frame'))
    assert np.array_equal(np.stack([f.copy() for f in rd]), ref)
    with pytest.raises(Y4MError, match='interlaced material is not supported'):
        M.infer_y4m(opt, io.BytesIO(data), io.BytesIO())
