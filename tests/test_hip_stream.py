"""FRNet.infer_stream / VSRModel.infer_stream / `--mode infer` on the GPU: the streamed frames equal
infer_sequence(pipeline=True) on the concatenated clip BIT FOR BIT -- the engine enqueues the same launches in the same
batch partition -- for every length and every way the input is chunked; memory does not grow with the length; a yielded
chunk stays valid until the generator is advanced; a time-out of the one-launch SRNet body is repaired per batch,
mid-stream, as often as it happens; an early close leaves the network usable.

Procedural weights and smooth_clip, as tests/test_hip_parity.py."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_DIR = os.path.join(ROOT_DIR, 'tests', 'golden')
from procedural_weights import generator_state_dict, smooth_clip

DEV = torch.device('cuda', 0)


def make_net(deg, s, precision='fp32'):
    from tecogan_pytorch_amd.models.networks import FRNet
    net = FRNet(3, 3, 64, 10, deg, s, precision=precision)
    net.load_state_dict(generator_state_dict(scale=s, degradation=deg), strict=True)
    return net.cuda().eval()


@pytest.fixture(scope='module')
def net4():
    return make_net('BD', 4)


def chunkings(clip):
    """frame by frame, in chunks of 3, as one chunk, in irregular chunks."""
    t = clip.shape[0]
    irregular, pos, sizes = [], 0, [2, 5, 1, 11, 3, 7]
    while pos < t:
        m = min(t - pos, sizes[len(irregular) % len(sizes)])
        irregular.append(clip[pos:pos + m])
        pos += m
    return {'frames': [f for f in clip], 'threes': [clip[i:i + 3] for i in range(0, t, 3)], 'one': [clip],
            'irregular': irregular}


def streamed(net, items, **kw):
    """The whole stream, each chunk copied out of its ring slot."""
    out = [c.copy() for c in net.infer_stream(iter(items), DEV, **kw)]
    assert all(c.dtype == np.uint8 and c.ndim == 4 for c in out)
    return np.concatenate(out, 0) if out else np.zeros((0,), np.uint8)


# ------------------------------------------------------------------ bit identity
@pytest.mark.parametrize('t', [1, 2, 9, 10, 17, 26, 60])
def test_stream_equals_infer_sequence_bit_for_bit(net4, t):
    clip = smooth_clip(t, 3, 24, 40, seed=11 + t)
    ref = net4.infer_sequence(clip, DEV)
    assert ref.shape == (t, 96, 160, 3)
    for name, items in chunkings(clip).items():
        got = streamed(net4, items)
        assert got.shape == ref.shape and np.array_equal(got, ref), (t, name)


def test_stream_chunks_are_the_engine_batches(net4):
    clip = smooth_clip(30, 3, 24, 40, seed=4)
    sizes = [len(c) for c in net4.infer_stream(iter(chunkings(clip)['threes']), DEV)]
    assert sizes == [9, 8, 8, 5]


def test_stream_is_lazy_and_bounded_ahead(net4):
    """Nothing is pulled before the first next(); never more than STREAM_SLOTS internal batches ahead of the yield."""
    from tecogan_pytorch_amd.models.networks import tecogan_nets as N
    clip = smooth_clip(60, 3, 24, 40, seed=4)
    pulled = []

    def source():
        for i in range(60):
            pulled.append(i)
            yield clip[i]
    gen = net4.infer_stream(source(), DEV)
    assert pulled == []
    first, later = N.stream_batch_sizes()
    yielded = 0
    for chunk in gen:
        assert len(pulled) - yielded <= first + (N.STREAM_SLOTS - 1) * later
        yielded += len(chunk)
    assert yielded == 60


def test_stream_2x_bi():
    net = make_net('BI', 2)
    clip = smooth_clip(19, 3, 24, 40, seed=8)
    ref = net.infer_sequence(clip, DEV)
    assert ref.shape == (19, 48, 80, 3)
    assert np.array_equal(streamed(net, chunkings(clip)['irregular']), ref)


def test_stream_full_size_uses_the_resident_launch(net4):
    import ctypes
    from tecogan_pytorch_amd import _lib
    clip = smooth_clip(20, 3, 134, 320, seed=2)
    ref = net4.infer_sequence(clip, DEV)
    got = streamed(net4, chunkings(clip)['threes'])
    assert np.array_equal(got, ref)
    lib = _lib.lib()
    plan = net4._get_plan(1, 134, 320, DEV)
    names = [lib.tg_frnet_kind_name(k).decode() for k in range(lib.tg_frnet_plan_kinds())]
    nl = ctypes.c_int()
    _lib.check(lib.tg_frnet_plan_kind_stats(plan.handle, names.index('conv3x3_wino_resident_kernel'), ctypes.byref(nl),
                                            None, None), 'kind_stats')
    assert nl.value == 1 and plan.chain_state() == (0, True)


def test_stream_fp16():
    net = make_net('BD', 4, precision='fp16')
    clip = smooth_clip(21, 3, 24, 40, seed=9)
    ref = net.infer_sequence(clip, DEV)
    assert np.array_equal(streamed(net, chunkings(clip)['threes']), ref)
    assert net._get_plan(1, 24, 40, DEV).precision == 'fp16'


def test_stream_uint8_hwc_input_equals_float_input(net4):
    """uint8 frames go up as bytes; the device divides by 255 exactly as `u8.float() / 255` does."""
    clip = smooth_clip(26, 3, 24, 40, seed=6)
    u8 = (clip.permute(0, 2, 3, 1) * 255.0).round().clamp(0, 255).to(torch.uint8).contiguous()
    as_float = (u8.float() / 255.0).permute(0, 3, 1, 2).contiguous()
    ref = net4.infer_sequence(as_float, DEV)
    assert np.array_equal(streamed(net4, [f for f in as_float]), ref)
    assert np.array_equal(streamed(net4, [f.numpy() for f in u8]), ref)               # what a decoder gives
    assert np.array_equal(streamed(net4, [u8[:7], u8[7:8], u8[8:]]), ref)
    assert np.array_equal(streamed(net4, [as_float[:5].cuda(), as_float[5:].cuda()]), ref)   # device-resident input


def test_stream_host_buffer_may_be_reused_by_the_caller(net4):
    """Host frames are copied when they are pulled: a decoder that decodes every frame into the same buffer is fine."""
    clip = smooth_clip(20, 3, 24, 40, seed=6)
    ref = net4.infer_sequence(clip, DEV)
    buf = torch.empty(3, 24, 40)

    def source():
        for i in range(20):
            buf.copy_(clip[i])
            yield buf
    assert np.array_equal(streamed(net4, source()), ref)


# ------------------------------------------------------------------ memory
def _pinned_in_use():
    """Bytes of pinned host memory in use, or None where this torch keeps no statistics of its pinned allocator."""
    if not hasattr(torch.cuda, 'host_memory_stats'):
        return None
    return torch.cuda.host_memory_stats().get('allocated_bytes.current')


def _peaks(fn):
    """(peak device bytes, most pinned bytes seen in use or None) of fn(sample); fn calls sample() wherever its pinned
    memory is at its largest.  The pinned allocator's own "peak" is not used: after reset_peak_host_memory_stats it
    read 222830813 bytes for a 40- and a 200-frame clip of either path alike.  The bytes in use are read instead,
    relative to what was in use before (other tests' arrays); the allocator's cache is emptied first, after an idle
    device and one small allocation that makes it look at the events of blocks it frees lazily, so a warmed cache
    cannot hide an allocation whichever way the allocator counts."""
    torch.cuda.synchronize()
    if _pinned_in_use() is not None:
        del_me = torch.empty(16, dtype=torch.uint8, pin_memory=True)
        del del_me
        empty = getattr(torch._C, '_host_emptyCache', None)
        if empty is not None:
            empty()
    base, seen = _pinned_in_use(), []
    torch.cuda.reset_peak_memory_stats()
    fn(lambda: seen.append(_pinned_in_use()))
    torch.cuda.synchronize()
    assert seen
    return torch.cuda.max_memory_allocated(), (None if base is None else max(seen) - base)


def test_stream_memory_does_not_grow_with_the_length(net4):
    hr_frame = 96 * 160 * 3                      # bytes of one HR uint8 frame

    def source(t):
        g = torch.Generator().manual_seed(t)
        left = t
        while left:                              # produced chunk by chunk, never held as a whole
            m = min(left, 5)
            yield torch.rand(m, 3, 24, 40, generator=g)
            left -= m

    def stream(t):
        def run(sample=lambda: None):
            n = 0
            for chunk in net4.infer_stream(source(t), DEV):
                n += len(chunk)
                sample()                         # (the rings are alive)
            assert n == t
        return run

    def whole(t):
        def run(sample=lambda: None):
            out = net4.infer_sequence(torch.cat(list(source(t)), 0), DEV)
            sample()                             # (the returned array is backed by the pinned clip buffer)
            assert len(out) == t
        return run
    for t in (40, 200):                          # plans of every batch size exist before anything is measured
        stream(t)()
        whole(t)()
    s40, s200 = _peaks(stream(40)), _peaks(stream(200))
    w40, w200 = _peaks(whole(40)), _peaks(whole(200))
    print('device peaks: stream 40/200 = %d / %d, infer_sequence 40/200 = %d / %d' % (s40[0], s200[0], w40[0], w200[0]))
    print('pinned peaks: stream 40/200 = %s / %s, infer_sequence 40/200 = %s / %s' % (s40[1], s200[1], w40[1], w200[1]))
    assert abs(s200[0] - s40[0]) <= hr_frame, (s40, s200)
    assert w200[0] - w40[0] >= 160 * hr_frame, (w40, w200)
    if s40[1] is not None:
        assert abs(s200[1] - s40[1]) <= hr_frame, (s40, s200)
        assert w200[1] - w40[1] >= 160 * hr_frame, (w40, w200)


# ------------------------------------------------------------------ ring validity
def test_yielded_chunk_is_valid_until_the_generator_is_advanced(net4):
    clip = smooth_clip(60, 3, 24, 40, seed=3)
    ref = net4.infer_sequence(clip, DEV)
    gen = net4.infer_stream(iter(chunkings(clip)['frames']), DEV)
    pos = 0
    for chunk in gen:
        mine = chunk.copy()
        torch.cuda.synchronize()                 # every batch in flight has finished, downloads included
        assert np.array_equal(chunk, mine), 'a batch in flight wrote into the slot the caller holds'
        assert np.array_equal(mine, ref[pos:pos + len(mine)])
        pos += len(mine)
    assert pos == 60


# ------------------------------------------------------------------ fail-safe (fresh processes: the launch forms are fixed by the environment)
_FAULT_HEAD = (
    "import sys, torch, warnings; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
    "import numpy as np\n"
    "from tests.test_hip_stream import make_net, streamed, DEV\n"
    "from procedural_weights import smooth_clip\n"
    "from tecogan_pytorch_amd import _lib\n"
    "H, W = 40, 72\n"
    "def fresh(rearm=None):\n"
    "    net = make_net('BD', 4)\n"
    "    plan = net._get_plan(1, H, W, DEV)\n"
    "    assert plan.chain_state() == (0, True), plan.chain_state()\n"
    "    if rearm is not None: plan.set_chain_rearm(rearm)\n"
    "    return net, plan\n"
    "limit = lambda plan, v: _lib.check(_lib.lib().tg_frnet_plan_set_chain_poll_limit(plan.handle, v), 'limit')\n"
    % (ROOT_DIR, GOLDEN_DIR))
# (TG_WINO_RES_CT=0: the first transposed conv is a launch of its own on the one-launch path and on the fallback alike,
# so the two paths agree bit for bit -- as in tests/test_hip_parity.py's fail-safe tests)
_FAULT_ENV = dict(TG_WINO_RES='1', TG_CONV_WINO='1', TG_WINO_RES_CT='0')


def _run(script, token):
    r = subprocess.run([sys.executable, '-c', _FAULT_HEAD + script], env=dict(os.environ, **_FAULT_ENV), timeout=600,
                       capture_output=True, text=True)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and token in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_one_injected_timeout_mid_stream_is_repaired():
    _run(
        "clip = smooth_clip(60, 3, H, W, seed=5)\n"
        "net, plan = fresh()\n"
        "clean = streamed(net, [f for f in clip])\n"
        "assert plan.chain_state() == (0, True) and np.array_equal(clean, net.infer_sequence(clip, DEV))\n"
        "net, plan = fresh()\n"
        "out = []\n"
        "with warnings.catch_warnings(record=True) as wl:\n"
        "    warnings.simplefilter('always')\n"
        "    gen = net.infer_stream(iter([f for f in clip]), DEV)\n"
        "    out.append(next(gen).copy())\n"
        "    limit(plan, -1)                       # every waiting workgroup of the bodies enqueued from here on gives up at once\n"
        "    out.append(next(gen).copy())          # (advancing enqueued one more batch: with the injection)\n"
        "    limit(plan, 1 << 21)                  # the co-tenant is gone again\n"
        "    for chunk in gen: out.append(chunk.copy())\n"
        "msgs = [str(w_.message) for w_ in wl if issubclass(w_.category, RuntimeWarning)]\n"
        "assert len(msgs) == 1 and 'computed again' in msgs[0], msgs\n"
        "got = np.concatenate(out, 0)\n"
        "assert got.shape == clean.shape and np.array_equal(got, clean), 'repaired stream differs'\n"
        "f, active = plan.chain_state(); assert f > 0 and not active, (f, active)\n"
        "assert np.array_equal(net.infer_sequence(clip[:7], DEV), clean[:7]), 'the network after the stream'\n"
        "print('faults', f, 'rearm', plan.rearm_state())\n"
        "print('STREAM-FAULT-OK')\n", 'STREAM-FAULT-OK')


def test_bodies_that_rearm_mid_stream_and_fault_again_are_repaired_each_time():
    _run(
        "clip = smooth_clip(80, 3, H, W, seed=7)\n"
        "net, plan = fresh()\n"
        "clean = streamed(net, [clip])\n"
        "net, plan = fresh(rearm=6)\n"
        "limit(plan, -1)                           # left on: every body that is armed again times out again\n"
        "with warnings.catch_warnings(record=True) as wl:\n"
        "    warnings.simplefilter('always')\n"
        "    gen = net.infer_stream(iter([f for f in clip]), DEV)\n"
        "    out = [next(gen).copy()]\n"
        "    eng = net._stream_ref()\n"
        "    for chunk in gen: out.append(chunk.copy())\n"
        "msgs = [str(w_.message) for w_ in wl if issubclass(w_.category, RuntimeWarning)]\n"
        "got = np.concatenate(out, 0)\n"
        "f, active = plan.chain_state(); rearms, wait = plan.rearm_state()\n"
        "print('faults', f, 'active', active, 'rearms', rearms, 'wait', wait, 'repairs', eng.reruns, 'warnings', len(msgs))\n"
        "assert got.shape == clean.shape and np.array_equal(got, clean), 'repaired stream differs'\n"
        "assert rearms >= 1 and eng.reruns >= 2, 'no re-armed body faulted inside the stream'\n"
        "assert eng.reruns <= 8 and wait >= 12, 'the back-off did not double'\n"
        "assert len(msgs) == 1, msgs\n"
        "print('STREAM-REARM-OK')\n", 'STREAM-REARM-OK')


def test_on_fault_raise_raises_at_the_batch():
    _run(
        "clip = smooth_clip(30, 3, H, W, seed=9)\n"
        "net, plan = fresh()\n"
        "ref = net.infer_sequence(clip, DEV)\n"
        "net, plan = fresh()\n"
        "limit(plan, -1)\n"
        "try:\n"
        "    streamed(net, [f for f in clip], on_fault='raise')\n"
        "    raise SystemExit('no error')\n"
        "except _lib.TecoganHipError as e:\n"
        "    assert 'timed out' in str(e), e\n"
        "limit(plan, 1 << 21)\n"
        "f, active = plan.chain_state(); assert f > 0 and not active, (f, active)\n"
        "assert np.array_equal(net.infer_sequence(clip, DEV), ref), 'the network after the raise'\n"
        "assert np.array_equal(streamed(net, [clip]), ref), 'the next stream'\n"
        "print('STREAM-RAISE-OK')\n", 'STREAM-RAISE-OK')


# ------------------------------------------------------------------ lifetime
def test_close_after_the_first_chunk_leaves_the_network_usable(net4):
    clip = smooth_clip(40, 3, 24, 40, seed=13)
    ref = net4.infer_sequence(clip, DEV)
    gen = net4.infer_stream(iter([f for f in clip]), DEV)
    first = next(gen).copy()
    gen.close()
    assert np.array_equal(first, ref[:len(first)])
    assert np.array_equal(net4.infer_sequence(clip, DEV), ref)
    assert np.array_equal(streamed(net4, [clip]), ref)


def test_second_live_stream_raises(net4):
    clip = smooth_clip(12, 3, 24, 40, seed=13)
    ref = net4.infer_sequence(clip, DEV)
    gen = net4.infer_stream(iter([f for f in clip]), DEV)
    first = next(gen).copy()
    with pytest.raises(RuntimeError, match='live stream'):
        net4.infer_stream(iter([clip]), DEV)
    rest = [c.copy() for c in gen]
    assert np.array_equal(np.concatenate([first] + rest, 0), ref)
    assert np.array_equal(streamed(net4, [clip]), ref)                  # exhausted: the next one opens


def test_input_errors_propagate_and_leave_the_network_usable(net4):
    clip = smooth_clip(40, 3, 24, 40, seed=14)
    ref = net4.infer_sequence(clip, DEV)

    class DecoderError(Exception):
        pass

    def broken():
        for i in range(25):
            yield clip[i]
        raise DecoderError('frame 25')
    got = []
    with pytest.raises(DecoderError):
        for chunk in net4.infer_stream(broken(), DEV):
            got.append(chunk.copy())
    if got:
        assert np.array_equal(np.concatenate(got, 0), ref[:sum(len(c) for c in got)])
    assert np.array_equal(net4.infer_sequence(clip, DEV), ref)

    def resized():
        for i in range(20):
            yield clip[i]
        yield torch.zeros(3, 24, 48)
    with pytest.raises(ValueError, match='size changed'):
        for chunk in net4.infer_stream(resized(), DEV):
            pass
    assert np.array_equal(streamed(net4, [clip]), ref)


# ------------------------------------------------------------------ the model wrapper and the CLI
def _opt(tmp_path=None):
    from tecogan_pytorch_amd.main import default_opt
    opt = default_opt()
    opt.update({'is_train': False, 'dist': False, 'device': 'cuda', 'rank': 0, 'world_size': 1})
    return opt


def test_vsr_model_infer_stream_equals_infer():
    from tecogan_pytorch_amd.models import define_model
    opt = _opt()
    assert opt['test'] == {'padding_mode': 'reflect', 'num_pad_front': 5}
    model = define_model(opt)
    model.net_G.load_state_dict(generator_state_dict(scale=4, degradation='BD'), strict=True)
    for t in (6, 23):
        clip = smooth_clip(t, 3, 24, 40, seed=20 + t)
        model.lr_data = clip
        ref = model.infer()
        assert ref.shape == (t, 96, 160, 3)
        got = np.concatenate([c.copy() for c in model.infer_stream(f for f in clip)], 0)
        assert got.shape == ref.shape and np.array_equal(got, ref), t
    with pytest.raises(ValueError, match='at least 6'):
        list(model.infer_stream(f for f in clip[:5]))
    model.lr_data = clip
    assert np.array_equal(model.infer(), ref)


def test_cli_infer_mode_writes_the_frames_of_vsr_model_infer(tmp_path):
    import yaml
    from PIL import Image
    from tecogan_pytorch_amd import main as M
    from tecogan_pytorch_amd.models import define_model
    pth = str(tmp_path / 'G_iter7.pth')
    torch.save(generator_state_dict(scale=4, degradation='BD'), pth)
    opt = M.default_opt()
    opt['model']['generator']['load_path'] = pth
    yml = str(tmp_path / 'infer.yml')
    with open(yml, 'w') as f:
        yaml.safe_dump(opt, f)
    src, dst = str(tmp_path / 'lr'), str(tmp_path / 'sr')
    clips = {}
    for name, t in (('calendar', 7), ('walk', 19)):
        clip = smooth_clip(t, 3, 24, 40, seed=len(name))
        u8 = (clip.permute(0, 2, 3, 1) * 255.0).round().clamp(0, 255).to(torch.uint8).contiguous()
        os.makedirs(os.path.join(src, name))
        for i in range(t):
            Image.fromarray(u8[i].numpy()).save(os.path.join(src, name, '%04d.png' % (i + 3)))
        clips[name] = u8
    M.main(['--mode', 'infer', '--opt', yml, '--input', src, '--output', dst])
    ref_opt = _opt()
    ref_opt['model']['generator']['load_path'] = pth
    model = define_model(ref_opt)
    for name, u8 in clips.items():
        model.lr_data = (u8.float() / 255.0).permute(0, 3, 1, 2)
        ref = model.infer()
        names = sorted(os.listdir(os.path.join(dst, name)))
        assert names == ['%04d.png' % (i + 3) for i in range(len(u8))]
        got = np.stack([np.asarray(Image.open(os.path.join(dst, name, n)).convert('RGB')) for n in names])
        assert got.shape == ref.shape and np.array_equal(got, ref), name
