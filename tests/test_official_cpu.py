"""CPU: the host side of the official evaluation protocol (metrics/official.py): crop arithmetic, file order,
frame ranges, the float32 aggregates against tests/golden/official.npz, the JSON schema, the `--mode test` switch
and the ABI of the two new kernels.  The kernels themselves are replaced here by numpy models of the same integer
arithmetic, so that the protocol's logic runs without a device; tests/test_hip_official.py checks the real ones."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import tecogan_pytorch_amd  # noqa: F401
from tecogan_pytorch_amd import _lib as L
from tecogan_pytorch_amd.metrics import official as O
from official_fixture import (CASES, CUTFR, DECOY_NAMES, FOLDER_CASES, clip_pair, crc, frame_file_names,
                              write_folder)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('tg_ssim_workspace_bytes', 'tg_ssim_y_u8', 'tg_psnr_yfloat_partials', 'tg_psnr_yfloat_sse_u8')


# ---- numpy models of the kernels (exact integer window sums, fp64 formula) ---------------------------------
def _yprime(a):
    a = a.astype(np.int64)
    return 65481 * a[..., 0] + 128553 * a[..., 1] + 24966 * a[..., 2]


def _box7(a):
    c = np.cumsum(np.cumsum(np.pad(a, ((1, 0), (1, 0))), 0), 1)
    return c[7:, 7:] - c[:-7, 7:] - c[7:, :-7] + c[:-7, :-7]


def ssim_model(true, pred, window):
    y, x, h, w = window
    out = []
    for t, p in zip(true.cpu().numpy(), pred.cpu().numpy()):
        X, Y = _yprime(t[y:y + h, x:x + w]), _yprime(p[y:y + h, x:x + w])
        Sx, Sy, Sxx, Syy, Sxy = _box7(X), _box7(Y), _box7(X * X), _box7(Y * Y), _box7(X * Y)
        D = 49.0 * 48.0 * 255000.0 ** 2
        vx, vy, vxy = (49 * Sxx - Sx * Sx) / D, (49 * Syy - Sy * Sy) / D, (49 * Sxy - Sx * Sy) / D
        ux, uy = Sx / (49 * 255000.0) + 16, Sy / (49 * 255000.0) + 16
        R = (Y.max() - Y.min()) / 255000.0
        C1, C2 = (0.01 * R) ** 2, (0.03 * R) ** 2
        out.append((((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))).mean())
    return torch.tensor(out, dtype=torch.float64)


def sse_model(true, pred, window):
    y, x, h, w = window
    return [int(((_yprime(t[y:y + h, x:x + w]) - _yprime(p[y:y + h, x:x + w])).astype(object) ** 2).sum())
            for t, p in zip(true.cpu().numpy(), pred.cpu().numpy())]


class FakeLPIPS:
    """The interface OfficialMetrics uses, on the CPU: five one-number 'taps' per frame."""
    scaling = True

    def __init__(self):
        self.frames_seen = 0

    def _chunk(self, t, h, w):
        return t

    def features_of(self, x):
        self.frames_seen += x.shape[0]
        m = x.float().mean(dim=(1, 2, 3)).view(-1, 1, 1, 1)
        return [m * (k + 1) for k in range(5)]

    def distance(self, a, b):
        return sum((u - v).abs().view(-1) for u, v in zip(a, b)) / 1000.0

    def __call__(self, a, b):
        return self.distance(self.features_of(a), self.features_of(b))


@pytest.fixture
def host_kernels(monkeypatch):
    from tecogan_pytorch_amd import ops
    monkeypatch.setattr(ops, 'ssim_y_u8', lambda t, p, window=None: ssim_model(t, p, window))
    monkeypatch.setattr(ops, 'psnr_yfloat_sse_u8', lambda t, p, window=None: sse_model(t, p, window))


# ---- crop, listing, frame range ----------------------------------------------------------------------------
@pytest.mark.parametrize('hw,exp', [((576, 720), (16, 8, 544, 704)), ((480, 720), (16, 8, 448, 704)),
                                    ((536, 1280), (12, 16, 512, 1248)), ((534, 1280), (11, 16, 512, 1248)),
                                    ((64, 96), (16, 16, 32, 64))])
def test_crop_8x8_table(hw, exp):
    assert O.crop_8x8_window(*hw) == exp
    assert O.OfficialMetrics.crop_8x8_window(*hw) == exp
    y, x, ch, cw = exp
    assert ch % 32 == 0 and cw % 32 == 0 and y >= 8 and x >= 8 and hw[0] - ch - y >= 8 and hw[1] - cw - x >= 8


def test_fixture_clips_are_the_goldens(golden):
    g = golden('official')
    assert list(g['cases']) == list(CASES) and int(g['cutfr']) == CUTFR
    for name in CASES:
        true, pred = clip_pair(name)
        assert [crc(true), crc(pred)] == g[f'{name}_crc'].tolist(), name
        assert g[f'{name}_range'].min() >= 50            # no frame near the 0/0 of a constant prediction


def test_list_png_order(tmp_path, golden):
    g = golden('official')
    for n in g['listing_files']:
        (tmp_path / str(n)).write_bytes(b'')
    got = [os.path.basename(p) for p in O.list_png(str(tmp_path))]
    assert got == [str(n) for n in g['listing_order']]
    assert got == frame_file_names(len(got)) and 'frame_10.png' in got
    assert got.index('frame_10.png') == got.index('frame_9.png') + 1
    assert not set(got) & set(DECOY_NAMES)


def test_frame_range():
    om = O.OfficialMetrics(device='cpu')
    assert om.keys == ('PSNR', 'SSIM') and om.skipped == ['tOF', 'LPIPS', 'tLP100']
    assert om.frame_range(7, 7) == (2, 5) and om.frame_range(7, 5) == (2, 5)
    assert om.frame_range(4, 4) == (2, 2) and om.frame_range(3, 0) == (2, 2)
    with pytest.raises(ValueError):
        om.frame_range(7, 4)
    assert O.OfficialMetrics(device='cpu', cutfr=0).frame_range(3, 3) == (0, 3)
    lp = FakeLPIPS()
    lp.scaling = False
    with pytest.raises(ValueError):
        O.OfficialMetrics(lp, device='cpu')


def test_compute_sequence_protocol_on_host(host_kernels, golden):
    """cutfr, both crops, PSNR / SSIM against upstream's values, tLP one shorter, chunking, feature reuse."""
    g = golden('official')
    for name in CASES:
        if 'vid4' in name:
            continue
        true, pred = clip_pair(name)
        lp = FakeLPIPS()
        r = O.OfficialMetrics(lp, device='cpu').compute_sequence(true, pred)
        n = true.shape[0] - 2 * CUTFR
        assert r['frames'] == true.shape[0] and r['evaluated'] == n and r['window'] == g[f'{name}_window'].tolist()
        assert [len(r[k]) for k in O.KEYS] == [n, n, n, n - 1]
        assert np.abs(np.array(r['SSIM']) - g[f'{name}_ssim']).max() <= 1e-9
        assert np.abs(np.array(r['PSNR']) / g[f'{name}_psnr'] - 1).max() <= 1e-12
        assert lp.frames_seen == 2 * n                      # every frame's taps once per side
        for chunk in (1, 2):
            r2 = O.OfficialMetrics(FakeLPIPS(), device='cpu', chunk_frames=chunk).compute_sequence(true, pred)
            assert r2 == r, chunk
        naive = FakeLPIPS()
        r3 = O.OfficialMetrics(naive, device='cpu', reuse_features=False).compute_sequence(true, pred)
        assert r3 == r and naive.frames_seen == 2 * n + 4 * (n - 1)
    same = O.OfficialMetrics(device='cpu').compute_sequence(true, true)
    assert same['PSNR'] == [float('inf')] * n and same['SSIM'] == [1.0] * n


def test_short_folder_is_empty_not_a_crash(host_kernels):
    true, pred = clip_pair(FOLDER_CASES[0])
    for t in (0, 1, 4):
        r = O.OfficialMetrics(FakeLPIPS(), device='cpu').compute_sequence(true[:t], pred[:t])
        assert [r[k] for k in O.KEYS] == [[], [], [], []] and r['evaluated'] == 0 and r['window'] is None
    r = O.OfficialMetrics(FakeLPIPS(), device='cpu').compute_sequence(true[:5], pred[:5])
    assert [len(r[k]) for k in O.KEYS] == [1, 1, 1, 0]
    with pytest.raises(ValueError):                          # 16 x 16 crops to nothing
        O.OfficialMetrics(device='cpu').compute_sequence(true[:, :16, :16], pred[:, :16, :16])


# ---- aggregates ----------------------------------------------------------------------------------------------
def _golden_lists(g, name):
    return {'PSNR': g[f'{name}_psnr'].tolist(), 'SSIM': g[f'{name}_ssim'].tolist(),
            'LPIPS': g[f'{name}_lpips32'].tolist(), 'tLP100': g[f'{name}_tlp32'].tolist()}


def test_aggregates_match_upstream_float32(golden):
    g = golden('official')
    agg = O.aggregate([O.folder_sums(_golden_lists(g, n)) for n in FOLDER_CASES])
    for k in O.KEYS:
        assert np.array_equal(np.float32(agg['Avg_' + k]), g['agg_Avg_' + k]), k
        assert agg['FolderAvg_' + k] == float(g['agg_FolderAvg_' + k]), k
        assert agg['FrameAvg_' + k] == float(g['agg_FrameAvg_' + k]), k
        assert agg['frame_counts'][k] == int(g['agg_count_' + k])
    # the averages are float32 arithmetic, not float64 means
    assert agg['FrameAvg_PSNR'] == float(np.float32(agg['FrameAvg_PSNR']))
    lines = O.summary_lines(agg)
    assert lines[0] == 'PSNR, total frame 5, total avg %02.4f, folder avg %02.4f' % (
        g['agg_FrameAvg_PSNR'], g['agg_FolderAvg_PSNR'])
    # what ranks exchange in --mode test (sums and counts) determines the same aggregates
    per_seq = {n: _golden_lists(g, n) for n in FOLDER_CASES}
    assert O.reduce_and_aggregate(per_seq, list(FOLDER_CASES), O.KEYS) == agg
    empty = O.aggregate([O.folder_sums({k: [] for k in O.KEYS})])
    assert np.isnan(empty['FrameAvg_PSNR']) and empty['frame_counts']['PSNR'] == 0


# ---- folders and JSON ------------------------------------------------------------------------------------------
def test_evaluate_folders_json_schema(tmp_path, host_kernels, golden, capsys):
    g = golden('official')
    res, tar = [], []
    for name in FOLDER_CASES:
        true, pred = clip_pair(name)
        tar.append(write_folder(tmp_path, f'gt_{name}', true))
        res.append(write_folder(tmp_path, f'sr_{name}', pred))
    om = O.OfficialMetrics(device='cpu')
    doc = om.evaluate_folders(res, tar, str(tmp_path / 'out'))
    assert json.load(open(tmp_path / 'out' / 'metrics.json')) == json.loads(json.dumps(doc))
    assert doc['skipped'] == ['tOF', 'LPIPS', 'tLP100'] and doc['keys'] == ['PSNR', 'SSIM'] and doc['cutfr'] == 2
    assert 'tOF' not in doc['folders'][0] and not any('tOF' in k for k in doc)
    assert doc['empty_folders'] == [] and [f['frames'] for f in doc['folders']] == [6, 7]
    assert [f['evaluated'] for f in doc['folders']] == [2, 3] and doc['folders'][0]['window'] == [16, 16, 32, 64]
    for f, name in zip(doc['folders'], FOLDER_CASES):      # the decoys and the name order did not disturb the frames
        assert np.abs(np.array(f['SSIM']) - g[f'{name}_ssim']).max() <= 1e-9
    for k in ('PSNR', 'SSIM'):
        assert doc['FrameAvg_' + k] == float(g['agg_FrameAvg_' + k])
        assert doc['FolderAvg_' + k] == float(g['agg_FolderAvg_' + k])
    text = (tmp_path / 'out' / 'metricsfile.txt').read_text()
    assert text == capsys.readouterr().out and text.startswith('PSNR, total frame 5, total avg 35.8402, folder avg')
    # a folder too short for cutfr: empty lists, reported, nan averages as numpy's 0/0 in the script
    true, pred = clip_pair(FOLDER_CASES[0])
    tar.append(write_folder(tmp_path, 'gt_short', true[:4]))
    res.append(write_folder(tmp_path, 'sr_short', pred[:4]))
    doc = om.evaluate_folders(res, tar, str(tmp_path / 'out'), quiet=True)
    assert doc['empty_folders'] == [2] and doc['folders'][2]['PSNR'] == [] and doc['frame_counts']['PSNR'] == 5
    assert np.isnan(doc['Avg_PSNR'][2]) and doc['FrameAvg_PSNR'] == float(g['agg_FrameAvg_PSNR'])
    assert (tmp_path / 'out' / 'metricsfile.txt').read_text().count('\n') == 4        # appended


def test_cli_arguments(tmp_path, capsys):
    with pytest.raises(SystemExit):
        O.main(['--results', 'a'])
    with pytest.raises(SystemExit):
        O.main(['--model', 'EDVR_BD'])
    assert O.main(['--model', 'TecoGAN_BD', '--results_root', str(tmp_path)]) == []     # no result folder: nothing to do
    assert O.EVAL_SETS == (('Vid4', ('calendar', 'city', 'foliage', 'walk')), ('ToS3', ('bridge', 'face', 'room')))


# ---- --mode test ---------------------------------------------------------------------------------------------
class _FakeModel:
    class net_G:
        @staticmethod
        def check_faults():
            pass

    def prepare_inference_data(self, data):
        self.gt = data['gt']

    def infer(self, device_output=False):
        return self.gt.clone()


class _FakeMC:
    def __init__(self, opt):
        self.calls = []

    def compute_sequence_metrics(self, *a):
        self.calls.append(a[0])

    def gather(self, ids):
        pass

    def display(self):
        pass


def test_mode_test_takes_the_old_path_without_the_key(monkeypatch, tmp_path, host_kernels):
    from tecogan_pytorch_amd import main as M
    from tecogan_pytorch_amd.metrics import metric_calculator
    monkeypatch.setattr(M, 'define_model', lambda opt: _FakeModel())
    monkeypatch.setattr(metric_calculator, 'MetricCalculator', _FakeMC)
    built = []

    def sentinel(opt):
        built.append(1)
        return O.OfficialMetrics(device='cpu')
    monkeypatch.setattr(M, '_official_metrics', sentinel)
    true, _ = clip_pair(FOLDER_CASES[0])
    seqs = [{'gt': torch.from_numpy(true), 'seq_idx': 'calendar'}]
    for topt in ({}, {'official_metrics': False}):
        opt = {'metric': {'PSNR': {}}, 'test': dict(topt, json_dir=str(tmp_path / 'json')), 'device': 'cpu'}
        mc = M.evaluate(opt, seqs, 'G_iter1', 'Vid4')
        assert mc.calls == ['calendar'] and not built and not (tmp_path / 'json').exists()
    opt['test']['official_metrics'] = True
    mc = M.evaluate(opt, seqs, 'G_iter1', 'Vid4')
    assert mc.calls == ['calendar'] and built == [1]
    doc = json.load(open(tmp_path / 'json' / 'Vid4_official.json'))
    assert doc['skipped'] == ['tOF', 'LPIPS', 'tLP100'] and doc['sequences'] == ['calendar']
    assert doc['frames'] == [6] and doc['evaluated'] == [2] and doc['windows'] == [[16, 16, 32, 64]]
    assert doc['FrameAvg_PSNR'] == float('inf') and doc['per_frame']['calendar']['SSIM'] == [1.0, 1.0]


# ---- ABI -------------------------------------------------------------------------------------------------------
def test_new_symbols_in_header_binding_and_library():
    text = open(os.path.join(ROOT, 'include', 'tecogan_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    declared = set(re.findall(r'\b(tg_[a-z0-9_]+)\s*\(', text))
    handle = ctypes.CDLL(L.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert s in declared and s in L.SIGNATURES and hasattr(handle, s), s
    lib = L.lib()
    assert lib.tg_ssim_workspace_bytes(1, 6, 64) == -1 and lib.tg_ssim_workspace_bytes(0, 64, 64) == -1
    assert lib.tg_ssim_workspace_bytes(3, 544, 704) == 3 * 8 + 3 * 34 * 11 * 8
    assert lib.tg_psnr_yfloat_partials(544, 704) == 94 and lib.tg_psnr_yfloat_partials(0, 4) == -1
    assert 2 ** 63 < 4096 * (255 * 219000) ** 2 < 2 ** 64   # the largest partial (4096 pixels) needs the unsigned range
    assert lib.tg_ssim_y_u8(None, None, 1, 8, 8, 8, 8, 0, 0, 8, 8, None, None, 0, None) == -2
    assert b'null' in lib.tg_last_error_string()
    assert lib.tg_psnr_yfloat_sse_u8(None, None, 1, 8, 8, 8, 8, 0, 0, 8, 8, None, None) == -2
    # shape errors (TG_E_SHAPE = -1) come back as codes before anything is launched: a window outside the smaller frame, no workspace
    one = ctypes.c_void_p(8)
    assert lib.tg_ssim_y_u8(one, one, 1, 64, 64, 60, 64, 0, 0, 64, 64, one, one, 1 << 20, None) == -1
    assert lib.tg_ssim_y_u8(one, one, 1, 64, 64, 64, 64, 1, 0, 64, 64, one, one, 1 << 20, None) == -1
    assert lib.tg_ssim_y_u8(one, one, 1, 64, 64, 64, 64, 0, 0, 64, 64, one, one, 8, None) == -2
    assert lib.tg_psnr_yfloat_sse_u8(one, one, 1, 64, 64, 64, 64, 0, 60, 8, 8, one, None) == -1
