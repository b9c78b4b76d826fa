"""Scene-cut reset of FRNet.infer_stream on the GPU: the detector through the C ABI against
tests/scene_cut_ref.py BIT FOR BIT (flags, SAD, histogram distance) at shapes that take both load forms, with guard
words around the outputs; the conditional fill; and the stream -- a frame at a cut is frame 0 of a clip of its own, so
from a cut on the stream yields the bytes of a stream over the new scene alone.

Clips: A = smooth_clip(la, seed 3), B = 1 - smooth_clip(lb, seed 7) at LR 24x40; tests/test_scene_cut_cpu.py shows from
the specification alone that the default thresholds fire at the joint and nowhere else."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from procedural_weights import generator_state_dict, smooth_clip
from tests import scene_cut_ref as R

ROOT_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device('cuda', 0)
GUARD = 0xA5


def make_net(deg, s, precision='fp32'):
    from tecogan_pytorch_amd.models.networks import FRNet
    net = FRNet(3, 3, 64, 10, deg, s, precision=precision)
    net.load_state_dict(generator_state_dict(scale=s, degradation=deg), strict=True)
    return net.cuda().eval()


@pytest.fixture(scope='module')
def net4():
    return make_net('BD', 4)


def two_scenes(la, lb):
    a, b = smooth_clip(la, 3, 24, 40, seed=3), 1.0 - smooth_clip(lb, 3, 24, 40, seed=7)
    return torch.cat([a, b], 0), b


def three_scenes():
    return torch.cat([smooth_clip(6, 3, 24, 40, seed=3), 1.0 - smooth_clip(7, 3, 24, 40, seed=7),
                      smooth_clip(9, 3, 24, 40, seed=5)], 0)


def chunkings(clip):
    """frame by frame, in chunks of 3, as one chunk, in irregular chunks (as tests/test_hip_stream.py)."""
    t = clip.shape[0]
    irregular, pos, sizes = [], 0, [2, 5, 1, 11, 3, 7]
    while pos < t:
        m = min(t - pos, sizes[len(irregular) % len(sizes)])
        irregular.append(clip[pos:pos + m])
        pos += m
    return {'frames': [f for f in clip], 'threes': [clip[i:i + 3] for i in range(0, t, 3)], 'one': [clip],
            'irregular': irregular}


def streamed(net, items, **kw):
    out = [c.copy() for c in net.infer_stream(iter(items), DEV, **kw)]
    return np.concatenate(out, 0)


def _guarded(nbytes, dtype, pad=16):
    buf = torch.full((pad + nbytes + pad,), GUARD, dtype=torch.uint8, device=DEV)
    return buf, buf[pad:pad + nbytes].view(dtype)


def _guards_intact(buf, pad=16):
    return bool((buf[:pad] == GUARD).all()) and bool((buf[-pad:] == GUARD).all())


# ------------------------------------------------------------------ 1. the detector equals the specification
def gpu_flags(frames, s_min, d_min, forced=None, detect=True, offset=4):
    """tg_scene_cut_flags through the C ABI on (n+1,3,h,w) float32 numpy; the frames start `offset` bytes past a 16-byte
    boundary, every output sits between guard words."""
    from tecogan_pytorch_amd import _lib as L
    lib = L.lib()
    n, _, h, w = frames.shape
    n -= 1
    raw = torch.zeros(16 + frames.nbytes + 16, dtype=torch.uint8, device=DEV)
    assert raw.data_ptr() % 16 == 0
    src = raw[offset:offset + frames.nbytes].view(torch.float32)
    src.copy_(torch.from_numpy(np.ascontiguousarray(frames)).reshape(-1))
    (bf, flags), (bs, sad), (bh, hd) = _guarded(4 * n, torch.int32), _guarded(8 * n, torch.int64), _guarded(4 * n, torch.int32)
    wsb = lib.tg_scene_cut_workspace_bytes(n)
    ws = torch.full((wsb,), GUARD, dtype=torch.uint8, device=DEV)           # (the call zeroes it itself)
    fm = None if forced is None else torch.from_numpy(np.asarray(forced, np.uint8)).to(DEV)
    L.check(lib.tg_scene_cut_flags(src.data_ptr(), n, h, w, int(s_min), int(d_min), None if fm is None else fm.data_ptr(),
                                   1 if detect else 0, flags.data_ptr(), sad.data_ptr(), hd.data_ptr(), ws.data_ptr(),
                                   wsb, torch.cuda.current_stream().cuda_stream), 'tg_scene_cut_flags')
    torch.cuda.synchronize()
    assert _guards_intact(bf) and _guards_intact(bs) and _guards_intact(bh), 'tg_scene_cut_flags wrote outside an output'
    return flags.cpu().numpy(), sad.cpu().numpy().view(np.uint64), hd.cpu().numpy().view(np.uint32)


def _detector_inputs(n, h, w, seed):
    rng = np.random.default_rng(seed)
    shape = (n + 1, 3, h, w)
    noise = rng.random(shape, dtype=np.float32)
    outside = noise.copy()
    outside[rng.random(shape) < 0.2] = -0.3
    outside[rng.random(shape) < 0.2] = 1.7
    nan = noise.copy()
    nan[n // 2 + (1 if n > 1 else 0), 1, h // 2, w // 2] = np.nan
    return {'smooth': smooth_clip(n + 1, 3, h, w, seed=seed).numpy(), 'noise': noise,
            'boundaries': ((rng.integers(0, 255, shape) + 0.5) / 255.0).astype(np.float32),
            'outside': outside, 'nan': nan}


def _same(got, ref):
    return all(g.dtype == r.dtype and np.array_equal(g, r) for g, r in zip(got, ref))


@pytest.mark.parametrize('n', [1, 3, 9])
@pytest.mark.parametrize('h,w', [(1, 1), (2, 2), (7, 5), (17, 23), (24, 40), (33, 130), (134, 320)])
def test_detector_is_bit_identical_to_the_specification(h, w, n):
    s_min, d_min = R.thresholds(R.MAD, R.HIST, h, w)
    inputs = _detector_inputs(n, h, w, seed=1000 * h + w + n)
    for name, frames in inputs.items():
        ref = R.flags(frames, s_min, d_min)
        for offset in (4, 0):                                   # scalar loads; 16-byte loads where h * w allows them
            got = gpu_flags(frames, s_min, d_min, offset=offset)
            assert _same(got, ref), (name, offset, got, ref)
    frames = inputs['noise']
    _, sad, hd = R.flags(frames, 0, 0)
    j = n - 1
    # the thresholds are inclusive, and both must hold
    for s, d, want in ((int(sad[j]), 0, 1), (int(sad[j]) + 1, 0, 0), (0, int(hd[j]), 1), (0, int(hd[j]) + 1, 0),
                       (int(sad[j]), int(hd[j]), 1), (int(sad[j]) + 1, int(hd[j]), 0)):
        got = gpu_flags(frames, s, d)
        assert _same(got, R.flags(frames, s, d)) and got[0][j] == want, (s, d, got)
    # a forced mask with the detector off comes back as it is; with it on, it is ORed in
    mask = (np.arange(n) % 2 == 0).astype(np.uint8)
    got = gpu_flags(frames, 0, 0, forced=mask, detect=False)
    assert np.array_equal(got[0], mask.astype(np.int32)) and _same(got, R.flags(frames, 0, 0, mask, False))
    hard = gpu_flags(frames, 1 << 40, 0, forced=mask, detect=True)
    assert np.array_equal(hard[0], mask.astype(np.int32))
    assert _same(gpu_flags(frames, 0, 0, forced=mask, detect=False), got)           # a second run: the same outputs


def test_ops_wrapper_equals_the_c_abi_and_refuses_cpu_tensors():
    from tecogan_pytorch_amd import _lib as L, ops
    frames = _detector_inputs(3, 24, 40, seed=5)['smooth']
    frames[2:] = 1.0 - frames[2:]
    ref = R.flags(frames, *R.thresholds(R.MAD, R.HIST, 24, 40))
    assert ref[0].tolist() == [0, 1, 0]
    f, s, d = ops.scene_cut_flags(torch.from_numpy(frames).to(DEV), R.MAD, R.HIST)
    assert (f.dtype, s.dtype, d.dtype) == (torch.int32, torch.int64, torch.int32)
    assert np.array_equal(f.cpu().numpy(), ref[0]) and np.array_equal(s.cpu().numpy().view(np.uint64), ref[1])
    assert np.array_equal(d.cpu().numpy().view(np.uint32), ref[2])
    f, _, _ = ops.scene_cut_flags(torch.from_numpy(frames).to(DEV), R.MAD, R.HIST, forced=[1, 0, 0], detect=False)
    assert f.tolist() == [1, 0, 0]
    with pytest.raises(L.TecoganHipError):
        ops.scene_cut_flags(torch.from_numpy(frames), R.MAD, R.HIST)
    with pytest.raises(L.TecoganHipError):
        ops.scene_cut_flags(torch.from_numpy(frames[:1]).to(DEV), R.MAD, R.HIST)
    with pytest.raises(L.TecoganHipError):
        ops.scene_cut_flags(torch.from_numpy(frames).to(DEV), R.MAD, R.HIST, forced=[1, 0])


# ------------------------------------------------------------------ 2. the conditional fill
@pytest.mark.parametrize('pad', [16, 5])                        # 5: the buffer starts off a 16-byte boundary
@pytest.mark.parametrize('nbytes', [16, 48, 3 * 8 * 12 * 4, 3 * 8 * 12 * 4 + 7, 3, 2 * 1024 * 1024 + 20])
def test_zero_if_flag_fills_exactly_the_bytes_or_nothing(nbytes, pad):
    from tecogan_pytorch_amd import _lib as L
    lib, st = L.lib(), torch.cuda.current_stream().cuda_stream
    pattern = (torch.arange(pad + nbytes + pad, device=DEV) % 251 + 1).to(torch.uint8)
    flag = torch.tensor([0, 1, -7], dtype=torch.int32, device=DEV)
    buf = pattern.clone()
    L.check(lib.tg_zero_if_flag(buf.data_ptr() + pad, nbytes, flag.data_ptr(), st), 'tg_zero_if_flag')
    assert torch.equal(buf, pattern)                            # flag 0: every byte as it was
    for k in (1, 2):                                            # any non-zero flag fills
        buf = pattern.clone()
        L.check(lib.tg_zero_if_flag(buf.data_ptr() + pad, nbytes, flag.data_ptr() + 4 * k, st), 'tg_zero_if_flag')
        assert not buf[pad:pad + nbytes].any()
        assert torch.equal(buf[:pad], pattern[:pad]) and torch.equal(buf[pad + nbytes:], pattern[pad + nbytes:])


# ------------------------------------------------------------------ 3. a cut on a batch border: exact
def _check_aligned_cut(net, all_chunkings=False):
    from tecogan_pytorch_amd.models.networks import SceneCut
    clip, b = two_scenes(8, 18)
    sc = SceneCut()
    out = streamed(net, [f for f in clip], scene_cut=sc)
    assert sc.cuts == [8] and sc.scores == []
    plain = streamed(net, [f for f in clip])
    alone = streamed(net, [f for f in b])
    assert out.shape == plain.shape and np.array_equal(out[:8], plain[:8])
    assert np.array_equal(out[8:], alone)                       # the second scene, as if the stream had started there
    assert not np.array_equal(out[8:], plain[8:])               # ... which the recurrence alone does not give
    forced = SceneCut(detect=False, at=[8])
    assert np.array_equal(streamed(net, [f for f in clip], scene_cut=forced), out) and forced.cuts == [8]
    if all_chunkings:
        for name, items in chunkings(clip).items():
            sc = SceneCut()
            assert np.array_equal(streamed(net, items, scene_cut=sc), out) and sc.cuts == [8], name
    return out


def test_cut_on_a_batch_border_restarts_the_stream_bit_for_bit(net4):
    _check_aligned_cut(net4, all_chunkings=True)


# ------------------------------------------------------------------ 4. a cut inside a batch
def test_cut_inside_a_batch(net4):
    """Frame 5 is the new scene's frame 0 bit for bit.  The frames behind it have their flows from a flow pass of
    another partition than the stream over B alone (frames 6..8 share batch 0's pass with scene A): the summation order
    of the batched FNet layers differs, the bound is the 1 level tests/test_hip_parity.py holds for the same cause.
    Measured on the MI355X: 0.0009 % of the bytes behind the cut differ, by 1 level (the share is printed)."""
    from tecogan_pytorch_amd.models.networks import SceneCut
    clip, b = two_scenes(5, 12)
    sc = SceneCut()
    out = streamed(net4, [f for f in clip], scene_cut=sc)
    alone = streamed(net4, [f for f in b])
    assert sc.cuts == [5]
    diff = np.abs(out[5:].astype(np.int16) - alone.astype(np.int16))
    print('cut inside a batch: %.4f %% of the bytes behind the cut differ from the stream over B alone, max %d level(s)'
          % (100.0 * (diff > 0).mean(), diff.max()))
    assert np.array_equal(out[5], alone[0])
    assert diff.max() <= 1


# ------------------------------------------------------------------ 5. three scenes
def test_three_scenes_under_every_chunking(net4):
    from tecogan_pytorch_amd.models.networks import SceneCut
    clip = three_scenes()
    outs = {}
    for name, items in chunkings(clip).items():
        sc = SceneCut()
        outs[name] = streamed(net4, items, scene_cut=sc)
        assert sc.cuts == [6, 13], name
    assert all(np.array_equal(o, outs['frames']) for o in outs.values())
    assert np.array_equal(outs['frames'][:6], streamed(net4, [f for f in clip])[:6])


# ------------------------------------------------------------------ 6. input kinds
def test_uint8_and_i420_input(net4):
    from tecogan_pytorch_amd import ops
    from tecogan_pytorch_amd.models.networks import SceneCut, Yuv420
    clip, _ = two_scenes(8, 18)
    u8 = (clip.permute(0, 2, 3, 1) * 255.0).round().clamp(0, 255).to(torch.uint8).contiguous()
    as_float = (u8.float() / 255.0).permute(0, 3, 1, 2).contiguous()
    a, b, c = SceneCut(keep_scores=True), SceneCut(keep_scores=True), SceneCut(keep_scores=True)
    ref = streamed(net4, [f for f in as_float], scene_cut=a)
    assert np.array_equal(streamed(net4, [f.numpy() for f in u8], scene_cut=b), ref)
    assert np.array_equal(streamed(net4, [as_float[:5].cuda(), as_float[5:].cuda()], scene_cut=c), ref)
    assert a.cuts == b.cuts == c.cuts == [8] and a.scores == b.scores == c.scores
    assert a.scores == R.stream_cuts(as_float.numpy())[1]
    spec = Yuv420(24, 40)
    i420 = ops.rgb_to_yuv420(u8.to(DEV), spec.matrix, spec.full_range, spec.siting).cpu().numpy()
    sc = SceneCut()
    out = np.concatenate([x.copy() for x in net4.infer_stream(iter([f for f in i420]), DEV, yuv=spec, scene_cut=sc)], 0)
    assert sc.cuts == [8] and out.shape == (26, spec.out_frame_bytes(4))
    # uint8 input with png and a forced cut: the files are those of the frames the same stream yields without png
    from tecogan_pytorch_amd.models.networks import Png
    d, e = SceneCut(detect=False, at=[8]), SceneCut(detect=False, at=[8])
    frames = streamed(net4, [f.numpy() for f in u8], scene_cut=d)
    files = [v.tobytes() for chunk in net4.infer_stream(iter([f.numpy() for f in u8]), DEV, png=Png(), scene_cut=e)
             for v in chunk]
    assert files == ops.png_encode(torch.from_numpy(frames).to(DEV)) and d.cuts == e.cuts == [8]


# ------------------------------------------------------------------ 7. the other networks
def test_cut_on_a_batch_border_2x_bi():
    assert _check_aligned_cut(make_net('BI', 2)).shape == (26, 48, 80, 3)


def test_cut_on_a_batch_border_fp16():
    net = make_net('BD', 4, precision='fp16')
    _check_aligned_cut(net)
    assert net._get_plan(1, 24, 40, DEV).precision == 'fp16'


# ------------------------------------------------------------------ 8. the model wrapper and the CLI
def _opt():
    from tecogan_pytorch_amd.main import default_opt
    opt = default_opt()
    opt.update({'is_train': False, 'dist': False, 'device': 'cuda', 'rank': 0, 'world_size': 1})
    return opt


def test_vsr_model_reports_the_cut_at_the_callers_index():
    from tecogan_pytorch_amd.models import define_model
    from tecogan_pytorch_amd.models.networks import SceneCut
    opt = _opt()
    assert opt['test']['num_pad_front'] == 5
    model = define_model(opt)
    model.net_G.load_state_dict(generator_state_dict(scale=4, degradation='BD'), strict=True)
    clip, _ = two_scenes(8, 18)
    sc = SceneCut(keep_scores=True)
    got = np.concatenate([c.copy() for c in model.infer_stream((f for f in clip), scene_cut=sc)], 0)
    assert sc.cuts == [8] and len(sc.scores) == 26
    padded = torch.cat([clip[1:6].flip(0), clip], 0)
    inner = SceneCut(keep_scores=True)
    ref = streamed(model.net_G, [f for f in padded], scene_cut=inner)
    assert inner.cuts == [13] and np.array_equal(got, ref[5:]) and sc.scores == inner.scores[5:]
    forced = SceneCut(detect=False, at=[0, 3])
    list(model.infer_stream((f for f in clip), scene_cut=forced))
    assert forced.cuts == [3]


def test_cli_y4m_with_scene_cut_writes_the_bytes_of_the_api_call(tmp_path):
    import yaml
    from tecogan_pytorch_amd import main as M, ops
    from tecogan_pytorch_amd.data.y4m import Y4MReader
    from tecogan_pytorch_amd.models import define_model
    from tecogan_pytorch_amd.models.networks import SceneCut, Yuv420
    pth = str(tmp_path / 'G_iter7.pth')
    torch.save(generator_state_dict(scale=4, degradation='BD'), pth)
    opt = M.default_opt()
    opt['model']['generator']['load_path'] = pth
    yml = str(tmp_path / 'infer.yml')
    with open(yml, 'w') as f:
        yaml.safe_dump(opt, f)
    clip, _ = two_scenes(8, 6)
    u8 = (clip.permute(0, 2, 3, 1) * 255.0).round().clamp(0, 255).to(torch.uint8).contiguous()
    spec = Yuv420(24, 40, 'bt601', True, 'center')
    i420 = ops.rgb_to_yuv420(u8.to(DEV), spec.matrix, spec.full_range, spec.siting).cpu().numpy()
    src, dst = str(tmp_path / 'in.y4m'), str(tmp_path / 'out.y4m')
    with open(src, 'wb') as f:
        f.write(b'YUV4MPEG2 W40 H24 F25:1 Ip A1:1 C420jpeg XYSCSS=420JPEG XCOLORRANGE=FULL\n')
        for fr in i420:
            f.write(b'FRAME\n' + fr.tobytes())
    M.main(['--mode', 'infer', '--opt', yml, '--input', src, '--output', dst, '--yuv-matrix', 'bt601', '--scene-cut'])
    data = open(dst, 'rb').read()
    got = np.stack([fr.copy() for fr in Y4MReader(io.BytesIO(data))])
    ref_opt = _opt()
    ref_opt['model']['generator']['load_path'] = pth
    model = define_model(ref_opt)
    sc = SceneCut()
    api = np.concatenate([c.copy() for c in model.infer_stream(iter([f for f in i420]), yuv=spec, scene_cut=sc)], 0)
    plain = np.concatenate([c.copy() for c in model.infer_stream(iter([f for f in i420]), yuv=spec)], 0)
    assert sc.cuts == [8] and got.shape == api.shape and np.array_equal(got, api) and not np.array_equal(got, plain)
    # --output -: stdout is the y4m stream and nothing else; the cuts are on stderr
    env = dict(os.environ, PYTHONPATH=ROOT_DIR + os.pathsep + os.environ.get('PYTHONPATH', ''))
    r = subprocess.run([sys.executable, '-m', 'tecogan_pytorch_amd.main', '--mode', 'infer', '--opt', yml, '--input', '-',
                        '--output', '-', '--yuv-matrix', 'bt601', '--scene-cut', '--scene-cut-mad', '24',
                        '--scene-cut-hist', '0.25'], input=open(src, 'rb').read(), cwd=ROOT_DIR, env=env,
                       capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout == data, (len(r.stdout), len(data), r.stdout[:80])
    assert b'scene cuts at frames [8]' in r.stderr


# ------------------------------------------------------------------ 9. the scores
def test_kept_scores_equal_the_specification(net4):
    from tecogan_pytorch_amd.models.networks import SceneCut
    clip = three_scenes()
    cuts, scores = R.stream_cuts(clip.numpy())
    sc = SceneCut(keep_scores=True)
    streamed(net4, chunkings(clip)['irregular'], scene_cut=sc)
    assert sc.cuts == cuts == [6, 13] and sc.scores == scores
    # thresholds nothing reaches: scored, never cut; the detector off: the forced ones alone
    high = SceneCut(mad=200.0, hist=0.9, at=[4, 21, 22, 99], keep_scores=True)
    streamed(net4, [clip], scene_cut=high)
    assert high.cuts == [4, 21] and high.scores == scores
