"""The device PNG encoder's LZ77 mode on the GPU: tg_png_encode_lz_u8 equals tests/png_lz_ref.py
BYTE FOR BYTE on every branch of the format, for a batch of different frames at an odd placement of `out` without
touching a byte outside its regions; lz77=False is the Huffman-only encoder's bytes; FRNet.infer_stream(png=Png(lz77=
True)) yields the LZ files of the frames the stream yields without `png`, and Png() what it always did.

Everything that touches the GPU runs in ONE child process, once, under a time limit, and reports a line per item; the
tests compare what it reported.  If the child ends by a signal, at its limit or with an error, nothing further is
started on the GPU from this module: every item it left unreported fails as 'not run'."""
import base64
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

pytestmark = pytest.mark.gpu

from tests import png_lz_ref as Z
from tests import png_ref as P

ROOT_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_DIR = os.path.join(ROOT_DIR, 'tests', 'golden')
MARK = 'PNG-LZ-ITEM '
CASES = Z.cases()
GUARD, OFFSET, EXTRA = 64, 3, 13                # the guard band, `out`'s odd byte offset, stride = capacity + 13
STREAM_T, STREAM_LR = 5, (24, 40)


def batch_frames():
    """Three frames of one size and of different kinds: LZ segments, a run across the cut, no match at all."""
    smooth = dict((c[0], c[1]) for c in CASES)['64x176 smooth']
    noise = np.random.RandomState(23).randint(0, 256, smooth.shape).astype(np.uint8)
    return [smooth, np.zeros_like(smooth), noise]


# ------------------------------------------------------------------ the child
def _report(name, **fields):
    rec = {k: ([base64.b64encode(b).decode() for b in v] if isinstance(v, list) and v and isinstance(v[0], bytes) else v)
           for k, v in fields.items()}
    print(MARK + json.dumps(dict(rec, name=name)), flush=True)


def child_main():
    import torch
    from procedural_weights import generator_state_dict, smooth_clip
    from tecogan_pytorch_amd import _lib as L
    from tecogan_pytorch_amd import ops
    from tecogan_pytorch_amd.models.networks import FRNet, Png
    dev = torch.device('cuda', 0)
    for name, img, filter in CASES:
        _report('case:' + name, files=ops.png_encode(torch.from_numpy(img).to(dev), filter, lz77=True))
    smooth = batch_frames()[0]
    x = torch.from_numpy(smooth).to(dev)
    _report('plain', files=ops.png_encode(x, 'adaptive', lz77=False) + ops.png_encode(x, 'adaptive') + ops.png_encode(x))
    # a batch of three through the C ABI, `out` at an odd offset, a guard band on either side
    frames = batch_frames()
    lib = L.lib()
    n, (h, w) = len(frames), frames[0].shape[:2]
    cap = lib.tg_png_capacity(h, w)
    stride = cap + EXTRA
    buf = torch.full((GUARD + OFFSET + n * stride + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    sizes = torch.zeros(n, dtype=torch.int64, device=dev)
    ws = torch.empty(lib.tg_png_lz_workspace_bytes(n, h, w), dtype=torch.uint8, device=dev)
    xs = torch.from_numpy(np.stack(frames)).to(dev)
    L.check(lib.tg_png_encode_lz_u8(xs.data_ptr(), n, h, w, L.PNG_FILTER['adaptive'], buf.data_ptr() + GUARD + OFFSET,
                                    stride, sizes.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream),
            'tg_png_encode_lz_u8')
    torch.cuda.synchronize()
    host, sizes = buf.cpu().numpy(), sizes.cpu().tolist()
    first = GUARD + OFFSET
    _report('batch', files=[host[first + k * stride:first + k * stride + sizes[k]].tobytes() for k in range(n)], sizes=sizes,
            cap=cap, before_ok=bool((host[:first] == 0xA5).all()), behind_ok=bool((host[first + n * stride:] == 0xA5).all()),
            behind=int(host[first + n * stride:].size))
    # the stream
    net = FRNet(3, 3, 64, 10, 'BD', 4)
    net.load_state_dict(generator_state_dict(scale=4, degradation='BD'), strict=True)
    net = net.cuda().eval()
    clip = smooth_clip(STREAM_T, 3, *STREAM_LR, seed=12)
    rgb = np.concatenate([c.copy() for c in net.infer_stream(iter([f for f in clip]), dev)], 0)
    files = lambda png: [v.tobytes() for chunk in net.infer_stream(iter([f for f in clip]), dev, png=png) for v in chunk]
    _report('stream', shape=list(rgb.shape), rgb=[rgb.tobytes()], lz=files(Png(lz77=True)), plain=files(Png()),
            ops_lz=ops.png_encode(torch.from_numpy(rgb).to(dev), lz77=True))


@pytest.fixture(scope='module')
def records():
    """{item: record} of the one child; `get(item)` fails as 'not run' for what the child did not report."""
    script = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
              "from tests.test_hip_png_lz import child_main\n"
              "child_main()\n" % (ROOT_DIR, GOLDEN_DIR))
    try:
        r = subprocess.run([sys.executable, '-c', script], capture_output=True, text=True, timeout=300)
        out, err, trouble = r.stdout, r.stderr, None if r.returncode == 0 else 'ended with status %d' % r.returncode
    except subprocess.TimeoutExpired as e:
        text = lambda s: s.decode(errors='replace') if isinstance(s, bytes) else (s or '')
        out, err, trouble = text(e.stdout), text(e.stderr), 'was killed at its time limit of %d s' % e.timeout
    recs = {}
    for line in out.splitlines():
        if line.startswith(MARK):
            try:
                d = json.loads(line[len(MARK):])
            except ValueError:                   # (a line cut short by the kill)
                continue
            recs[d['name']] = {k: ([base64.b64decode(b) for b in v] if isinstance(v, list) and v and isinstance(v[0], str)
                                   else v) for k, v in d.items()}

    def get(item):
        if item not in recs:
            pytest.fail('not run: the child %s\n%s\n%s' % (trouble or 'did not report %s' % item, out[-1000:], err[-4000:]),
                        pytrace=False)
        return recs[item]
    return get


_REF = {}


def ref(img, filter):
    key = (img.shape, img.tobytes(), filter)
    if key not in _REF:
        _REF[key] = Z.encode(img, filter)
    return _REF[key]


def same(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    assert got == want, (what, next(i for i in range(len(want)) if got[i] != want[i]))


def decode(png):
    with Image.open(io.BytesIO(bytes(png))) as im:
        assert im.mode == 'RGB'
        return np.asarray(im).copy()


# ------------------------------------------------------------------ the tests
@pytest.mark.parametrize('name,img,filter', CASES, ids=[c[0] for c in CASES])
def test_png_encode_lz77_equals_the_specification_byte_for_byte(name, img, filter, records):
    got, = records('case:' + name)['files']
    same(got, ref(img, filter), name)
    assert len(got) <= len(P.encode(img, filter))
    assert np.array_equal(decode(got), img)


def test_a_batch_at_an_odd_offset_and_nothing_outside_is_written(records):
    rec = records('batch')
    frames = batch_frames()
    assert rec['cap'] == P.capacity(*frames[0].shape[:2])
    for k, frame in enumerate(frames):
        assert rec['sizes'][k] == len(ref(frame, 'adaptive')), k
        same(rec['files'][k], ref(frame, 'adaptive'), k)
    assert ref(frames[2], 'adaptive') == P.encode(frames[2], 'adaptive')                  # no match: the Huffman-only file
    assert rec['before_ok'] and rec['behind_ok'] and rec['behind'] == GUARD


def test_lz77_false_is_the_huffman_only_encoder(records):
    smooth = batch_frames()[0]
    want = P.encode(smooth, 'adaptive')
    files = records('plain')['files']
    assert len(files) == 3
    for got in files:
        same(got, want, 'lz77=False')
    assert len(ref(smooth, 'adaptive')) < len(want)


def test_stream_yields_the_lz_files_of_the_frames_it_yields_without_png(records):
    rec = records('stream')
    t, (h, w) = STREAM_T, (4 * STREAM_LR[0], 4 * STREAM_LR[1])
    assert rec['shape'] == [t, h, w, 3]
    flen = h * (3 * w + 1)
    assert P.SEG < flen < 2 * P.SEG and P.SEG % (3 * w + 1) != 0                          # two segments, the cut mid-row
    rgb = np.frombuffer(rec['rgb'][0], np.uint8).reshape(t, h, w, 3)
    assert len(rec['lz']) == len(rec['plain']) == len(rec['ops_lz']) == t
    for k in range(t):
        same(rec['lz'][k], rec['ops_lz'][k], ('stream against ops', k))
        assert np.array_equal(decode(rec['lz'][k]), rgb[k]), k                           # the order is the frames'
        same(rec['plain'][k], P.encode(rgb[k], 'adaptive'), ('Png()', k))
        assert len(rec['lz'][k]) <= len(rec['plain'][k]), k
    for k in (0, t - 1):
        same(rec['lz'][k], ref(rgb[k], 'adaptive'), ('stream against the specification', k))
