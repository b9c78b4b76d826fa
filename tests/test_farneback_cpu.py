"""CPU: the specification of tOF's optical flow (tests/farneback_ref.py) tested as what it
claims to be -- an optical flow -- plus its exact zeros and geometry, and the host side of the opt-in: key orders,
`skipped` lists, the JSON note, the unchanged warning path, and the ABI's argument checks (no kernel is launched)."""
import ctypes
import json
import logging

import numpy as np
import pytest
import torch

import tecogan_pytorch_amd  # noqa: F401
from tecogan_pytorch_amd import _lib as L
from tecogan_pytorch_amd.metrics import official as O
from tecogan_pytorch_amd.metrics.metric_calculator import MetricCalculator
from tests import farneback_ref as F
from tests.farneback_fixture import shifted_texture, sequence_pair


# ---- the specification is an optical flow --------------------------------------------------------------------
@pytest.mark.parametrize('shift', [(1.5, -0.75), (6.0, 3.0), (0.3, 0.2)])
def test_known_motion(shift):
    """A smooth texture (Gaussian-filtered noise, sigma 2) rendered with a sub-pixel shift by cubic interpolation, at
    256 x 264 (all four levels): the interior mean end-point error, 16 pixels in, is at most 0.02 px."""
    a, b = shifted_texture(256, 264, shift, seed=1)
    flow = F.farneback(a, b)
    epe = np.sqrt(((flow - np.array(shift)) ** 2).sum(-1))[16:-16, 16:-16].mean()
    print(f'known motion {shift}: interior mean EPE {epe:.4f} px')
    assert epe <= 0.02


def test_exact_zeros():
    a, _ = shifted_texture(72, 100, (1.0, 0.0), seed=2)
    const = np.full((40, 56), 200, np.uint8)
    for dt in (np.float64, np.float32):
        assert not F.farneback(a, a, dt).any()                     # identical frames
        assert not F.farneback(const, const, dt).any()             # constant frames
        assert not F.polyexp(const.astype(dt), dt)[[0, 1, 4]].any()  # the antisymmetric sums of a constant region
    true, pred = sequence_pair(72, 100, 4, seed=3)
    assert (F.tof(true, true) == 0).all() and (F.tof(true, true, official=False) == 0).all()
    assert (F.tof(true, pred) > 0).all()


def test_alt32_is_float32_and_close():
    a, b = shifted_texture(72, 100, (2.25, -1.5), seed=4)
    f64, f32 = F.farneback(a, b), F.alt32(a, b)
    assert f64.dtype == np.float64 and f32.dtype == np.float32
    rel = np.linalg.norm(f32 - f64) / np.linalg.norm(f64)
    assert 0 < rel < 1e-4, rel


# ---- geometry ------------------------------------------------------------------------------------------------
def test_geometry():
    assert [F.top_level(*s) for s in ((40, 56), (72, 100), (256, 264), (63, 200), (64, 64), (576, 720))] == \
        [0, 1, 3, 0, 1, 3]
    assert F.level_size(75, 101, 1) == (38, 50) and F.level_size(72, 100, 1) == (36, 50)
    assert F.level_size(256, 264, 3) == (32, 33) and F.level_size(75, 101, 0) == (75, 101)
    assert [len(F.blur_taps(k)) for k in range(4)] == [3, 3, 9, 19]
    assert F.blur_taps(0).tolist() == [0.25, 0.5, 0.25]
    for k in range(1, 4):
        assert abs(F.blur_taps(k).sum() - 1) < 1e-15
    rgb = np.array([[[255, 255, 255], [0, 0, 0], [255, 0, 0], [0, 255, 0], [0, 0, 255], [12, 200, 77]]], np.uint8)
    assert F.gray_u8(rgb).tolist() == [[255, 0, 76, 150, 29, 130]]


def test_library_geometry_matches_the_specification():
    """tg_fb_level_size is host arithmetic: the library's level rule and half-even sizes against the numpy rule."""
    lib = L.lib()
    lh, lw = ctypes.c_int(), ctypes.c_int()
    for h, w in ((40, 56), (72, 100), (75, 101), (256, 264), (63, 200), (64, 64), (576, 720), (134, 321), (17, 16)):
        top = lib.tg_fb_level_size(h, w, 0, ctypes.byref(lh), ctypes.byref(lw))
        assert top == F.top_level(h, w) and (lh.value, lw.value) == (h, w)
        for k in range(4):
            assert lib.tg_fb_level_size(h, w, k, ctypes.byref(lh), ctypes.byref(lw)) == top
            assert (lh.value, lw.value) == F.level_size(h, w, k), (h, w, k)
    from tecogan_pytorch_amd import ops
    assert ops.farneback_levels(256, 264) == [(256, 264), (128, 132), (64, 66), (32, 33)]
    assert ops.farneback_levels(75, 101) == [(75, 101), (38, 50)]


def test_abi_argument_checks():
    lib = L.lib()
    lh = ctypes.c_int()
    assert lib.tg_fb_level_size(15, 64, 0, ctypes.byref(lh), ctypes.byref(lh)) == -2
    assert lib.tg_fb_level_size(64, 64, 4, ctypes.byref(lh), ctypes.byref(lh)) == -2
    assert lib.tg_fb_level_size(64, 64, 0, None, None) == -2
    assert lib.tg_farneback_workspace_bytes(1, 15, 64) == -1 and lib.tg_farneback_workspace_bytes(0, 64, 64) == -1
    one, two = lib.tg_farneback_workspace_bytes(1, 72, 100), lib.tg_farneback_workspace_bytes(2, 72, 100)
    assert 0 < one < two and one >= 72 * 100 * (2 + 8 + 8 + 40 + 20)
    assert lib.tg_farneback_flow_u8(None, 2, 72, 100, 72, 100, None, None, 0, None) == -2
    assert b'null' in lib.tg_last_error_string()
    # with (never dereferenced) non-null pointers: sizes and the workspace are checked before anything is launched
    p = ctypes.c_void_p(256)
    assert lib.tg_farneback_flow_u8(p, 2, 72, 100, 15, 100, p, p, 1 << 40, None) == -2      # h < 16
    assert lib.tg_farneback_flow_u8(p, 2, 72, 100, 72, 101, p, p, 1 << 40, None) == -2      # region outside the frame
    assert lib.tg_farneback_flow_u8(p, 1, 72, 100, 72, 100, p, p, 1 << 40, None) == -2      # one frame: no pair
    assert lib.tg_farneback_flow_u8(p, 2, 72, 100, 72, 100, p, p, one - 1, None) == -2      # short workspace
    assert b'workspace' in lib.tg_last_error_string()
    for fn, args in ((lib.tg_fb_gray_u8, (None, 1, 16, 16, 16, 16, None, None)),
                     (lib.tg_fb_level_image, (None, 1, 16, 16, 0, None, None, None)),
                     (lib.tg_fb_polyexp, (None, 1, 16, 16, None, None)),
                     (lib.tg_fb_update_matrices, (None, None, None, 1, 16, 16, None)),
                     (lib.tg_fb_blur_solve, (None, None, None, 1, 16, 16, None)),
                     (lib.tg_fb_resize_flow, (None, 16, 16, None, 32, 32, 1, None)),
                     (lib.tg_flow_epe_mean, (None, None, 1, 16, 16, 0, 0, 16, 16, None, None))):
        assert fn(*args) == -2, fn
    assert lib.tg_fb_polyexp(p, 1, 15, 16, p, None) == -2 and lib.tg_fb_level_image(p, 1, 40, 56, 1, p, p, None) == -2
    assert lib.tg_flow_epe_mean(p, p, 1, 16, 16, 1, 0, 16, 16, p, None) == -2             # window outside
    from tecogan_pytorch_amd import ops
    with pytest.raises(L.TecoganHipError):
        ops.farneback_flow(torch.zeros(2, 32, 32, 3, dtype=torch.uint8))
    with pytest.raises(L.TecoganHipError):
        ops.tof(torch.zeros(2, 32, 32, 3, dtype=torch.uint8), torch.zeros(2, 32, 32, 3, dtype=torch.uint8))


# ---- host logic of the opt-in --------------------------------------------------------------------------------
class FakeLPIPS:
    scaling = True

    def _chunk(self, t, h, w):
        return t

    def features_of(self, x):
        m = x.float().mean(dim=(1, 2, 3)).view(-1, 1, 1, 1)
        return [m * (k + 1) for k in range(5)]

    def distance(self, a, b):
        return sum((u - v).abs().view(-1) for u, v in zip(a, b)) / 1000.0

    def __call__(self, a, b):
        return self.distance(self.features_of(a), self.features_of(b))


def test_official_keys_and_skipped():
    assert O.KEYS == ('PSNR', 'SSIM', 'LPIPS', 'tLP100') and O.SKIPPED == ('tOF',)       # the constants stay
    assert O.KEYS_TOF == F.KEYS_OFFICIAL == ('PSNR', 'SSIM', 'LPIPS', 'tOF', 'tLP100')
    om = O.OfficialMetrics(FakeLPIPS(), device='cpu')
    assert om.keys == O.KEYS and om.skipped == ['tOF'] and om.tof is False
    om = O.OfficialMetrics(device='cpu')
    assert om.keys == ('PSNR', 'SSIM') and om.skipped == ['tOF', 'LPIPS', 'tLP100']
    om = O.OfficialMetrics(FakeLPIPS(), device='cpu', tof=True)
    assert om.keys == ('PSNR', 'SSIM', 'LPIPS', 'tOF', 'tLP100') and om.skipped == []
    om = O.OfficialMetrics(device='cpu', tof=True)
    assert om.keys == ('PSNR', 'SSIM', 'tOF') and om.skipped == ['LPIPS', 'tLP100']


@pytest.fixture
def host_kernels(monkeypatch):
    """The device kernels replaced by stand-ins, so that the protocol's host logic runs here; tOF is the
    specification itself, and a call of it without the opt-in fails the test."""
    from tecogan_pytorch_amd import ops
    calls = []
    monkeypatch.setattr(ops, 'ssim_y_u8', lambda t, p, window=None: torch.full((t.shape[0],), 0.5, dtype=torch.float64))
    monkeypatch.setattr(ops, 'psnr_yfloat_sse_u8', lambda t, p, window=None: [10 ** 15] * t.shape[0])

    def tof(t, p, window=None):
        calls.append(window)
        return torch.from_numpy(F.tof(t.numpy(), p.numpy(), official=window is not None))
    monkeypatch.setattr(ops, 'tof', tof)
    return calls


def test_official_host_logic(host_kernels, tmp_path):
    true, pred = sequence_pair(72, 100, 7, seed=5, pred_size=(74, 100))
    plain = O.OfficialMetrics(FakeLPIPS(), device='cpu').compute_sequence(true, pred)
    assert list(plain)[:4] == list(O.KEYS) and 'tOF' not in plain and not host_kernels
    om = O.OfficialMetrics(FakeLPIPS(), device='cpu', tof=True)
    r = om.compute_sequence(true, pred)
    assert list(r)[:5] == list(O.KEYS_TOF)
    assert len(r['tOF']) == 7 - 2 * 2 - 1 == len(r['tLP100']) and len(r['PSNR']) == 3
    assert host_kernels == [O.crop_8x8_window(72, 100)]
    assert r['tOF'] == F.tof(true[2:5], pred[2:5]).tolist()
    for k in O.KEYS:                                                   # the other columns do not move
        assert r[k] == plain[k]
    # too few frames: empty lists, no flow call
    short = om.compute_sequence(true[:5], pred[:5])
    assert short['tOF'] == [] and len(short['PSNR']) == 1 and len(host_kernels) == 1
    sums = O.folder_sums(r, om.keys)
    agg = O.aggregate([sums], om.keys)
    assert agg['frame_counts']['tOF'] == 2 and list(agg['frame_counts']) == list(O.KEYS_TOF)
    assert [ln.split(',')[0] for ln in O.summary_lines(agg, om.keys)] == list(O.KEYS_TOF)
    assert O.OfficialMetrics(device='cpu', tof=True).compute_sequence(true, pred)['tOF'] == r['tOF']
    with pytest.raises(ValueError):
        O.OfficialMetrics(device='cpu', tof=True, cutfr=0).compute_sequence(true[:, :15], pred[:, :15])


def test_official_json_note(host_kernels, tmp_path, monkeypatch):
    from tecogan_pytorch_amd.data import folder_dataset
    true, pred = sequence_pair(72, 100, 6, seed=6)
    store = {}
    for name, seq in (('gt', true), ('out', pred)):
        d = tmp_path / name
        d.mkdir()
        for i, f in enumerate(seq):
            (d / f'{i:03d}.png').write_bytes(b'')
            store[str(d / f'{i:03d}.png')] = f
    monkeypatch.setattr(folder_dataset, 'read_rgb', lambda p: store[str(p)])
    doc = O.OfficialMetrics(device='cpu', tof=True).evaluate_folders([str(tmp_path / 'out')], [str(tmp_path / 'gt')],
                                                                     str(tmp_path / 'log'), quiet=True)
    saved = json.load(open(tmp_path / 'log' / 'metrics.json'))
    assert saved['tOF_flow'] == doc['tOF_flow'] == 'farneback, restated, not compared with OpenCV'
    assert saved['keys'] == ['PSNR', 'SSIM', 'tOF'] and saved['skipped'] == ['LPIPS', 'tLP100']
    assert len(saved['folders'][0]['tOF']) == 1 and len(saved['Avg_tOF']) == 1
    plain = O.OfficialMetrics(device='cpu').evaluate_folders([str(tmp_path / 'out')], [str(tmp_path / 'gt')],
                                                             str(tmp_path / 'log2'), quiet=True)
    assert 'tOF_flow' not in plain and plain['skipped'] == ['tOF', 'LPIPS', 'tLP100']
    assert not any('tOF' in k for k in plain)


def test_cli_has_the_switch():
    with pytest.raises(SystemExit):
        O.main(['--tof'])                                              # parsed; fails on the missing folders only
    import inspect
    assert "tof=args.tof" in inspect.getsource(O.main)


def test_metric_calculator_warning_path_unchanged(caplog):
    """Without `backend: hip` a tOF section warns once and is left out, as before."""
    for cfg in ({'colorspace': 'y'}, None, {}, {'backend': 'opencv'}):
        caplog.clear()
        with caplog.at_level(logging.WARNING, logger='tecogan_pytorch_amd'):
            mc = MetricCalculator({'device': 'cpu', 'metric': {'PSNR': {'colorspace': 'y'}, 'tOF': cfg}})
        assert list(mc.metric_opt) == ['PSNR']
        assert sum('tOF' in r.getMessage() for r in caplog.records) == 1


def test_metric_calculator_backend_hip(host_kernels, caplog, tmp_path, monkeypatch):
    from tecogan_pytorch_amd.metrics import metric_calculator as MC
    monkeypatch.setattr(MC, 'compute_psnr_device', lambda t, p, cs: [30.0] * t.shape[0])
    with caplog.at_level(logging.WARNING, logger='tecogan_pytorch_amd'):
        mc = MetricCalculator({'device': 'cpu', 'metric': {'PSNR': {'colorspace': 'y'}, 'tOF': {'backend': 'hip'}}})
    assert list(mc.metric_opt) == ['PSNR', 'tOF'] and not any('tOF' in r.getMessage() for r in caplog.records)
    true, pred = sequence_pair(40, 56, 3, seed=7, pred_size=(40, 60))
    mc.compute_sequence_metrics('clip', true, pred)
    assert host_kernels == [None]                                      # the whole size-matched frame
    got = mc.metric_dict['clip']
    assert len(got['PSNR']) == 3 and got['tOF'] == F.tof(true, pred, official=False).tolist() and len(got['tOF']) == 2
    mc.gather(['clip'])
    assert mc.average()['tOF'] == pytest.approx(np.mean(got['tOF']))
    mc.save('G_iter10', str(tmp_path / 'm.json'))
    assert json.load(open(tmp_path / 'm.json'))['G_iter10']['tOF'] == f"{np.mean(got['tOF']):.6f}"
