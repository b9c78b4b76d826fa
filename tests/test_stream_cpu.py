"""Host logic of FRNet.infer_stream / VSRModel.infer_stream / `--mode infer` (no GPU): the batch partition without
knowing the length, the lazy front padding, input normalisation, ring-slot bookkeeping, the CLI's arguments and its
folder listing / output naming."""
import os

import numpy as np
import pytest
import torch

import tecogan_pytorch_amd  # noqa: F401
from tecogan_pytorch_amd.models.networks import tecogan_nets as N
from tecogan_pytorch_amd.models.base_model import BaseModel, front_pad_stream


def partition_of_infer_sequence(tot_frm, fnet_batch, k=1):
    """Independent restatement of the batch list _infer_sequence built by hand before clip_batches(t,
    *stream_batch_sizes(fb, k)) took its place: it is told the length and clamps to it."""
    nb_ = max(1, min(max(1, fnet_batch // k), tot_frm))
    nb0 = max(1, min(nb_, max(1, N.FNET_FIRST_PASS_FRAMES // k)))
    batches, i0 = [], 0
    while i0 < tot_frm:
        cnt = min(nb0 + 1 if not batches else nb_, tot_frm - i0)
        batches.append((i0, cnt))
        i0 += cnt
    return batches


def streamed_partition(chunks, fnet_batch):
    first, later = N.stream_batch_sizes(fnet_batch)
    sizes = {}
    for b, off, piece, full in N.stream_rebatch(N.stream_parts(iter(chunks)), first, later):
        assert off == sizes.get(b, 0), 'pieces of a batch are handed out in order, without gaps'
        sizes[b] = off + piece.shape[0]
        assert full == (sizes[b] == (first if b == 0 else later))
    out, i0 = [], 0
    for b in range(len(sizes)):
        out.append((i0, sizes[b]))
        i0 += sizes[b]
    return out


@pytest.mark.parametrize('fnet_batch', [1, 2, 4, 8, 16])
def test_partition_equals_infer_sequence_without_knowing_the_length(fnet_batch):
    rng = np.random.RandomState(fnet_batch)
    for t in range(1, 101):
        frames = torch.zeros(t, 3, 2, 2)
        assert streamed_partition([f for f in frames], fnet_batch) == partition_of_infer_sequence(t, fnet_batch)
        assert streamed_partition([frames], fnet_batch) == partition_of_infer_sequence(t, fnet_batch)
        cuts, pos = [], 0
        while pos < t:
            m = min(t - pos, int(rng.randint(1, 7)))
            cuts.append(frames[pos:pos + m])
            pos += m
        assert streamed_partition(cuts, fnet_batch) == partition_of_infer_sequence(t, fnet_batch)


@pytest.mark.parametrize('k', [1, 2, 4, 8])
def test_clip_batches_equal_the_restatement_for_lockstep_clips(k):
    for fnet_batch in (1, 2, 3, 4, 5, 8, 12, 16, 32):
        for t in range(1, 101):
            assert N.clip_batches(t, *N.stream_batch_sizes(fnet_batch, k)) == partition_of_infer_sequence(t, fnet_batch, k)


def test_batch_sizes_follow_the_environment(monkeypatch):
    monkeypatch.delenv('TG_FNET_BATCH', raising=False)
    assert N.stream_batch_sizes() == (9, 8)
    monkeypatch.setenv('TG_FNET_BATCH', '16')
    assert N.stream_batch_sizes() == (9, 16)
    monkeypatch.setenv('TG_FNET_BATCH', '2')
    assert N.stream_batch_sizes() == (3, 2)


def test_rebatch_pulls_lazily():
    """The next input item is asked for only when the previous one has been handed out entirely."""
    pulled = []

    def source():
        for i in range(40):
            pulled.append(i)
            yield torch.zeros(3, 2, 2)
    it = N.stream_rebatch(N.stream_parts(source()), 9, 8)
    for n in range(1, 21):
        next(it)
        assert len(pulled) == n


# ------------------------------------------------------------------ front padding
class _Pad(BaseModel):
    def __init__(self, mode, n_pad):
        self.opt = {'test': {'padding_mode': mode, 'num_pad_front': n_pad}}


@pytest.mark.parametrize('mode', ['reflect', 'replicate'])
@pytest.mark.parametrize('n_pad', [0, 5])
@pytest.mark.parametrize('form', ['f32', 'u8'])
def test_lazy_front_padding_equals_pad_sequence(mode, n_pad, form):
    g = torch.Generator().manual_seed(3)
    for t in (n_pad + 1, n_pad + 2, 13):
        if form == 'f32':
            clip = torch.rand(t, 3, 4, 6, generator=g)
        else:
            clip = (torch.rand(t, 4, 6, 3, generator=g) * 255).to(torch.uint8)
        ref, n = _Pad(mode, n_pad).pad_sequence(clip)
        assert n == n_pad
        for chunks in ([f for f in clip], [clip], [clip[:2], clip[2:3], clip[3:]] if t > 3 else [clip[:1], clip[1:]]):
            got = torch.cat(list(front_pad_stream(iter(chunks), mode, n_pad)), 0)
            assert got.dtype == ref.dtype and torch.equal(got, ref), (mode, n_pad, t)


def test_lazy_front_padding_buffers_no_more_than_it_needs():
    pulled = []

    def source():
        for i in range(30):
            pulled.append(i)
            yield torch.full((3, 2, 2), float(i))
    it = front_pad_stream(source(), 'reflect', 5)
    prefix = next(it)
    assert len(pulled) == 6 and [int(v) for v in prefix[:, 0, 0, 0]] == [5, 4, 3, 2, 1]
    head = next(it)
    assert len(pulled) == 6 and head.shape[0] == 6
    next(it)
    assert len(pulled) == 7


@pytest.mark.parametrize('mode', ['reflect', 'replicate'])
def test_lazy_front_padding_refuses_a_short_stream(mode):
    clip = torch.rand(5, 3, 4, 6)
    with pytest.raises(ValueError, match='at least 6'):
        list(front_pad_stream(iter([clip]), mode, 5))
    with pytest.raises(ValueError, match='at least 6'):
        list(front_pad_stream(iter([]), mode, 5))
    assert list(front_pad_stream(iter([]), mode, 0)) == []
    with pytest.raises(ValueError, match='padding mode'):
        list(front_pad_stream(iter([clip]), 'circular', 2))


# ------------------------------------------------------------------ input normalisation
def test_both_layouts_and_dtypes_are_accepted():
    u8 = np.zeros((4, 6, 3), np.uint8)
    for item, kind, shape in ((u8, 'u8', (1, 4, 6, 3)), (np.stack([u8] * 2), 'u8', (2, 4, 6, 3)),
                              (torch.from_numpy(u8), 'u8', (1, 4, 6, 3)),
                              (torch.zeros(3, 4, 6), 'f32', (1, 3, 4, 6)), (torch.zeros(5, 3, 4, 6), 'f32', (5, 3, 4, 6)),
                              (np.zeros((3, 4, 6), np.float32), 'f32', (1, 3, 4, 6))):
        k, x = N.stream_frames(item)
        assert k == kind and tuple(x.shape) == shape and torch.is_tensor(x)


def test_wrong_rank_dtype_and_channels_are_rejected():
    for bad in (np.zeros((4, 6), np.uint8), np.zeros((1, 1, 4, 6, 3), np.uint8), torch.zeros(6),
                torch.zeros(2, 2, 3, 4, 6), np.zeros((4, 6, 3), np.float64), torch.zeros(3, 4, 6, dtype=torch.float16),
                np.zeros((4, 6, 4), np.uint8), torch.zeros(4, 6, 3), [[1, 2, 3]], None):
        with pytest.raises(ValueError):
            N.stream_frames(bad)


def test_mid_stream_size_or_form_change_is_rejected_before_the_item_is_used():
    ok = [torch.zeros(3, 4, 6), torch.zeros(2, 3, 4, 6)]
    assert sum(x.shape[0] for _, x in N.stream_parts(iter(ok))) == 3
    seen = []
    with pytest.raises(ValueError, match='size changed'):
        for _, x in N.stream_parts(iter(ok + [torch.zeros(3, 4, 8)])):
            seen.append(x.shape[0])
    assert seen == [1, 2]
    with pytest.raises(ValueError, match='form of the first'):
        list(N.stream_parts(iter([torch.zeros(3, 4, 6), np.zeros((4, 6, 3), np.uint8)])))
    with pytest.raises(ValueError, match='size changed'):
        list(N.stream_parts(iter([np.zeros((4, 6, 3), np.uint8), np.zeros((6, 4, 3), np.uint8)])))
    # an empty chunk is skipped, not an error
    assert [x.shape[0] for _, x in N.stream_parts(iter([torch.zeros(0, 3, 4, 6), torch.zeros(3, 4, 6)]))] == [1]


# ------------------------------------------------------------------ ring slots
def test_ring_slot_bookkeeping():
    ring = N.StreamRing(3)
    assert N.STREAM_SLOTS == 3 and not ring.full()
    recs = [ring.submit(9), ring.submit(8), ring.submit(8)]
    assert recs == [(0, 0, 9), (1, 9, 8), (2, 17, 8)] and ring.full()
    assert len({ring.slot(b) for b, _, _ in ring.inflight}) == 3        # batches in flight never share a slot
    with pytest.raises(RuntimeError):
        ring.submit(8)
    assert ring.oldest() == (0, 0, 9) and ring.retire() == (0, 0, 9) and not ring.full()
    nxt = ring.submit(5)
    assert nxt == (3, 25, 5) and ring.slot(3) == ring.slot(0)           # the retired batch's slot is the one reused
    assert [r[0] for r in ring.inflight] == [1, 2, 3]
    # the flow-slot rule of the engine: batch b waits for the batch that used flow slot b & 1 before it, b - 2,
    # whose event lives in another ring slot than b's own
    for b in range(2, 50):
        assert ring.slot(b - 2) != ring.slot(b)


def test_one_stream_per_network_without_a_gpu():
    """The live-stream rule is host state: a second open raises at the call; a stream that was closed, or dropped
    before it ever ran, does not block the next."""
    net = N.FRNet(3, 3, 64, 10, 'BD', 4)
    g1 = net.infer_stream(iter([]), device='cpu')
    with pytest.raises(RuntimeError, match='live stream'):
        net.infer_stream(iter([]), device='cpu')
    assert list(g1) == []                       # an empty input: nothing to yield, nothing allocated
    g2 = net.infer_stream(iter([]), device='cpu')
    del g2                                      # never started
    g3 = net.infer_stream(iter([]), device='cpu')
    g3.close()
    with pytest.raises(ValueError, match='on_fault'):
        net.infer_stream(iter([]), device='cpu', on_fault='ignore')
    net.infer_stream(iter([]), device='cpu')


# ------------------------------------------------------------------ slot layouts of the form objects
@pytest.mark.parametrize('m,cnt', [(1, 1), (3, 1), (3, 3)])
def test_png_slot_layout(m, cnt):
    """A PNG slot is m int64 sizes, then m regions of `stride` bytes (the capacity rounded up to 8), file k from the
    first byte of region k: result() cuts exactly the first cnt files out of a hand-built pinned ring, as views."""
    from tecogan_pytorch_amd.models.networks.stream import Png, _PngOut
    ns, cap = 3, 21
    stride = 24
    out = _PngOut(Png())
    out.layout(m, cap)
    assert (out.png_stride, out.slot_bytes) == (stride, 8 * m + m * stride)
    sizes = np.array([[(0, stride, 5)[(sl + k) % 3] for k in range(m)] for sl in range(ns)], np.int64)
    ring = (np.arange(ns * (8 * m + m * stride)) % 251).astype(np.uint8).reshape(ns, 8 * m + m * stride)
    for sl in range(ns):
        ring[sl, :8 * m] = np.frombuffer(sizes[sl].tobytes(), np.uint8)
    assert {0, stride} <= set(sizes.ravel().tolist())
    want = ring.copy()
    out.host_out = torch.from_numpy(ring)
    for sl in range(ns):
        files = out.result(sl, cnt)
        assert isinstance(files, list) and len(files) == cnt
        for k, f in enumerate(files):
            lo = 8 * m + k * stride
            assert f.dtype == np.uint8 and f.shape == (int(sizes[sl, k]),)
            assert np.array_equal(f, want[sl, lo:lo + int(sizes[sl, k])])
            if f.size:                              # a view of the ring at exactly that offset, not a copy
                assert f.__array_interface__['data'][0] == ring[sl].__array_interface__['data'][0] + lo
    assert np.array_equal(ring, want)


@pytest.mark.parametrize('m,cnt', [(1, 1), (3, 1), (3, 3)])
def test_scene_cut_record_layout(m, cnt):
    """A slot's result record is m uint64 SADs at byte 0, m int32 flags at 8 m, m uint32 histogram distances at 12 m:
    report() hands the first cnt of each to SceneCut.report, and reset() is the address of the slot's flags."""
    from tecogan_pytorch_amd.models.networks.stream import SceneCut, _CutSlots
    ns, n_pixels, i0 = 3, 10, 17
    sc = SceneCut(keep_scores=True)
    slots = _CutSlots(sc)
    slots.layout(m)
    assert slots.slot_bytes == 16 * m
    sad = np.array([[1000 * sl + 10 * k + 2 ** 40 for k in range(m)] for sl in range(ns)], np.uint64)
    flags = np.array([[(sl + k) % 2 for k in range(m)] for sl in range(ns)], np.int32)
    dist = np.array([[7 * sl + k + 1 for k in range(m)] for sl in range(ns)], np.uint32)
    rec = np.zeros((ns, 16 * m), np.uint8)
    for sl in range(ns):
        rec[sl, :8 * m] = np.frombuffer(sad[sl].tobytes(), np.uint8)
        rec[sl, 8 * m:12 * m] = np.frombuffer(flags[sl].tobytes(), np.uint8)
        rec[sl, 12 * m:] = np.frombuffer(dist[sl].tobytes(), np.uint8)
    slots.sc_host, slots.n_pixels = torch.from_numpy(rec), n_pixels
    for sl in range(ns):
        sc.cuts.clear()
        sc.scores.clear()
        slots.report(sl, i0, cnt)
        assert sc.cuts == [i0 + k for k in range(cnt) if flags[sl, k]]
        assert sc.scores == [(int(sad[sl, k]) / n_pixels, int(dist[sl, k]) / (2 * n_pixels)) for k in range(cnt)]
    slots.sc_out, slots.hr_bytes = torch.zeros(ns, 16 * m, dtype=torch.uint8), 4 * 3 * 96 * 160
    for sl in range(ns):
        assert slots.reset(sl) == (slots.sc_out.data_ptr() + sl * 16 * m + 8 * m, 4 * 3 * 96 * 160)


# ------------------------------------------------------------------ CLI
def test_parse_args_accepts_the_infer_mode():
    from tecogan_pytorch_amd.main import parse_args
    a = parse_args(['--mode', 'infer', '--input', 'lr', '--output', 'sr', '--precision', 'fp16'])
    assert (a.mode, a.input, a.output, a.precision) == ('infer', 'lr', 'sr', 'fp16')
    a = parse_args(['--mode', 'test'])
    assert a.input is None and a.output is None


def _touch(path):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    open(path, 'wb').close()


def test_folder_listing_and_output_naming(tmp_path):
    from tecogan_pytorch_amd import main as M
    flat = str(tmp_path / 'flat')
    for n in ('0002.png', '0000.png', '0001.JPG', 'notes.txt'):
        _touch(os.path.join(flat, n))
    _touch(os.path.join(flat, 'sub', '0000.png'))                       # frames directly inside: sub-folders are ignored
    seqs = M.infer_sequences(flat)
    assert [s for s, _ in seqs] == [''] and [os.path.basename(p) for p in seqs[0][1]] == ['0000.png', '0001.JPG', '0002.png']
    out = str(tmp_path / 'out')
    assert [M.infer_output_path(flat, out, '', p) for p in seqs[0][1]] == \
        [os.path.join(out, '', n) for n in ('0000.png', '0001.png', '0002.png')]
    nested = str(tmp_path / 'nested')
    for s, n in (('walk', '0001.png'), ('walk', '0000.png'), ('city', 'a/0000.png'), ('city', 'b/0000.png'), ('empty', 'x.txt')):
        _touch(os.path.join(nested, s, n))
    seqs = M.infer_sequences(nested)
    assert [s for s, _ in seqs] == ['city', 'walk']
    assert [M.infer_output_path(nested, out, s, p) for s, fl in seqs for p in fl] == \
        [os.path.join(out, 'city', 'a', '0000.png'), os.path.join(out, 'city', 'b', '0000.png'),
         os.path.join(out, 'walk', '0000.png'), os.path.join(out, 'walk', '0001.png')]
    assert M.infer_sequences(str(tmp_path / 'nested' / 'empty')) == []
    assert 1 <= M.INFER_WRITER_THREADS <= 8


def test_infer_mode_writers_copy_out_of_the_slot_before_it_is_reused(tmp_path, monkeypatch):
    """main.infer with a stand-in model whose infer_stream yields views of ONE buffer that it overwrites as soon as it
    is advanced (the ring-slot contract at its harshest): every PNG written must still hold its own frame, under the
    input's name, for both folder layouts; frames are decoded lazily."""
    from PIL import Image
    from tecogan_pytorch_amd import main as M
    decoded = []

    class Model:
        class net_G:
            @staticmethod
            def check_faults():
                pass

        def infer_stream(self, frames):
            slot = np.zeros((4, 16, 24, 3), np.uint8)
            n = 0
            for f in frames:                                  # 2x nearest-neighbour "super-resolution"
                decoded.append(n)
                slot[n % 4] = np.repeat(np.repeat(f, 2, 0), 2, 1)
                n += 1
                if n % 4 == 0:
                    yield slot[:4]
                    slot[:] = 0
            if n % 4:
                yield slot[:n % 4]
                slot[:] = 0
    monkeypatch.setattr(M, 'define_model', lambda opt: Model())
    rng = np.random.RandomState(0)
    src, dst = str(tmp_path / 'lr'), str(tmp_path / 'sr')
    frames = {}
    for seq, t in (('a', 10), ('b', 3)):
        os.makedirs(os.path.join(src, seq))
        for i in range(t):
            f = rng.randint(0, 256, (8, 12, 3)).astype(np.uint8)
            Image.fromarray(f).save(os.path.join(src, seq, 'im%03d.png' % i))
            frames[(seq, 'im%03d.png' % i)] = f
    done = M.infer({}, src, dst)
    assert done == {'a': 10, 'b': 3}
    for (seq, name), f in frames.items():
        got = np.asarray(Image.open(os.path.join(dst, seq, name)).convert('RGB'))
        assert np.array_equal(got, np.repeat(np.repeat(f, 2, 0), 2, 1)), (seq, name)
    # the flat layout, into a folder of its own
    done = M.infer({}, os.path.join(src, 'b'), str(tmp_path / 'flat'))
    assert done == {'': 3} and sorted(os.listdir(str(tmp_path / 'flat'))) == ['im000.png', 'im001.png', 'im002.png']
    os.makedirs(str(tmp_path / 'nothing'))
    with pytest.raises(ValueError, match='no png'):
        M.infer({}, str(tmp_path / 'nothing'), dst)
