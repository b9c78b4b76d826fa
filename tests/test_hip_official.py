"""GPU: the official evaluation protocol on the device (csrc/tg_ssim.hip, metrics/official.py) against the upstream
script's own values (tests/golden/official.npz, make_golden_official.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from lpips_fixture import alexnet_state_dict
from official_fixture import CASES, CUTFR, FOLDER_CASES, clip_pair, write_folder

pytestmark = pytest.mark.gpu

DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def ops():
    from tecogan_pytorch_amd import ops as o
    return o


def _lin_sd(golden):
    g = golden('lpips')
    return {f'lin{k}.model.1.weight': torch.from_numpy(g[f'lin{k}']) for k in range(5)}


@pytest.fixture(scope='module')
def lpips(golden):
    """LPIPS with ScalingLayer, as the official script runs it."""
    import tecogan_pytorch_amd  # noqa: F401
    from tecogan_pytorch_amd.metrics.lpips import LPIPS
    m = LPIPS(device=DEV, scaling=True)
    m.load_alexnet_state_dict(alexnet_state_dict())
    m.load_lin_state_dict(_lin_sd(golden))
    return m


def _evaluated(name):
    """The frames of a case the protocol evaluates, on the device, and their window."""
    from tecogan_pytorch_amd.metrics.official import crop_8x8_window
    true, pred = clip_pair(name)
    t = torch.from_numpy(true[CUTFR:true.shape[0] - CUTFR]).to(DEV)
    p = torch.from_numpy(pred[CUTFR:pred.shape[0] - CUTFR]).to(DEV)
    win = crop_8x8_window(min(t.shape[1], p.shape[1]), min(t.shape[2], p.shape[2]))
    return t, p, win


def b(v):
    """The bound of tests/test_hip_lpips.py::test_lpips_matches_reference_fp64: the reference's own fp32 accuracy
    with ~10x room."""
    return 2e-4 * np.abs(v) + 1e-9


def test_ssim_matches_golden(ops, golden):
    """|kernel - upstream fp64| <= 1e-9 on every evaluated frame of every case.  Two fp64 evaluations of the formula
    (scipy's order vs exact integer window sums) differ by ~1e-13; an fp32 accumulation misses by >= 1e-8.
    Measured maximum on the MI355X: 1.01e-14 (case d1, frame 4); a numpy model of the same integer arithmetic gives
    the same figure."""
    g = golden('official')
    worst = 0.0
    for name in CASES:
        t, p, win = _evaluated(name)
        assert list(win) == g[f'{name}_window'].tolist()
        got = ops.ssim_y_u8(t, p, win).cpu().numpy()
        err = np.abs(got - g[f'{name}_ssim'])
        print(f'ssim {name}: {got} max abs err {err.max():.3e}')
        worst = max(worst, float(err.max()))
        assert got.dtype == np.float64 and np.all(err <= 1e-9), (name, got, g[f'{name}_ssim'])
    print(f'ssim: measured maximum {worst:.3e}')
    vals = np.concatenate([g[f'{n}_ssim'] for n in CASES])
    assert vals.min() < 0.8 and vals.max() > 0.98             # the cases span a range of values


def test_ssim_window_batch_and_rerun_bit_for_bit(ops):
    for name in ('b_130x170_blur', 'c_vid4_576x720_noise40', 'a_96x128_noise8'):
        t, p, win = _evaluated(name)
        y, x, h, w = win
        full = ops.ssim_y_u8(t, p, win)
        tc, pc = t[:, y:y + h, x:x + w].contiguous(), p[:, y:y + h, x:x + w].contiguous()
        assert torch.equal(full, ops.ssim_y_u8(tc, pc)), name                     # window vs a copy of the crop
        one = torch.cat([ops.ssim_y_u8(t[i:i + 1], p[i:i + 1], win) for i in range(t.shape[0])])
        assert torch.equal(full, one), name                                       # batched vs one per call
        assert torch.equal(full, ops.ssim_y_u8(t, p, win)), name                  # run to run
        assert ops.psnr_yfloat_sse_u8(t, p, win) == ops.psnr_yfloat_sse_u8(tc, pc)
    # windows that are not multiples of the tile, at odd origins
    t, p, _ = _evaluated('b_130x170_blur')
    for win in ((3, 5, 7, 7), (1, 2, 23, 71), (0, 0, 128, 168), (40, 90, 17, 65)):
        y, x, h, w = win
        a = ops.ssim_y_u8(t, p, win)
        c = ops.ssim_y_u8(t[:, y:y + h, x:x + w].contiguous(), p[:, y:y + h, x:x + w].contiguous())
        assert torch.equal(a, c) and bool(torch.isfinite(a).all()), win
    from tecogan_pytorch_amd._lib import TecoganHipError
    with pytest.raises(TecoganHipError):
        ops.ssim_y_u8(t, p, (0, 0, 129, 168))                 # outside the smaller frame
    with pytest.raises(TecoganHipError):
        ops.ssim_y_u8(t, p, (0, 0, 6, 64))


def test_ssim_identical_and_constant_frames(ops):
    t, _, win = _evaluated('a_96x128_noise8')
    assert ops.ssim_y_u8(t, t, win).tolist() == [1.0] * t.shape[0]
    # a constant prediction: data_range 0; it returns (NaN where numpy has 0/0 at flat positions) and does not hang
    flat = torch.full_like(t, 77)
    out = ops.ssim_y_u8(flat, flat, win).cpu()
    assert out.shape == (t.shape[0],) and bool(torch.isnan(out).all())
    assert bool(torch.isfinite(ops.ssim_y_u8(flat, t, win)).all())


def test_psnr_yfloat_matches_golden(ops, golden):
    from tecogan_pytorch_amd.metrics.official import OfficialMetrics
    g = golden('official')
    om = OfficialMetrics(device=DEV)
    for name in CASES:
        true, pred = clip_pair(name)
        r = om.compute_sequence(true, pred)
        rel = np.abs(np.array(r['PSNR']) / g[f'{name}_psnr'] - 1.0)
        print(f'psnr {name}: {r["PSNR"]} max rel err {rel.max():.3e}')
        assert np.all(rel <= 1e-12), (name, r['PSNR'], g[f'{name}_psnr'])
        t, p, win = _evaluated(name)
        # the device sums are the exact integers
        y, x, h, w = win
        d = (t[:, y:y + h, x:x + w].cpu().numpy().astype(np.int64) -
             p[:, y:y + h, x:x + w].cpu().numpy().astype(np.int64)) @ np.array([65481, 128553, 24966])
        assert ops.psnr_yfloat_sse_u8(t, p, win) == [int((f.astype(object) ** 2).sum()) for f in d]
        same = om.compute_sequence(true, true)
        assert same['PSNR'] == [float('inf')] * (true.shape[0] - 2 * CUTFR)
    # the largest possible partial does not wrap: black against white
    z = torch.zeros(1, 64, 64, 3, dtype=torch.uint8, device=DEV)
    assert ops.psnr_yfloat_sse_u8(z, z + 255) == [64 * 64 * (255 * 219000) ** 2]


def test_lpips_and_tlp_match_golden_fp64(lpips, golden):
    from tecogan_pytorch_amd.metrics.official import OfficialMetrics
    g = golden('official')
    om = OfficialMetrics(lpips, device=DEV)
    for name in CASES:
        true, pred = clip_pair(name)
        r = om.compute_sequence(torch.from_numpy(true).to(DEV), torch.from_numpy(pred).to(DEV))
        ref, tref = g[f'{name}_lpips64'], g[f'{name}_tlp64']
        # upstream's own fp32 values are within the bound
        assert np.all(np.abs(g[f'{name}_lpips32'] - ref) <= b(ref)), name
        tb = 100.0 * (b(g[f'{name}_dgt64']) + b(g[f'{name}_dout64']))
        assert np.all(np.abs(g[f'{name}_tlp32'] - tref) <= tb), name
        lp, tlp = np.array(r['LPIPS']), np.array(r['tLP100'])
        print(f'lpips {name}: {lp} err/bound {np.max(np.abs(lp - ref) / b(ref)):.3f}; tlp {tlp} err/bound '
              f'{np.max(np.abs(tlp - tref) / tb) if len(tb) else 0:.3f}')
        assert lp.shape == ref.shape and np.all(np.abs(lp - ref) <= b(ref)), (name, lp, ref)
        assert tlp.shape == tref.shape and np.all(np.abs(tlp - tref) <= tb), (name, tlp, tref)


def test_feature_reuse_changes_nothing_and_is_real(lpips, ops, monkeypatch):
    from tecogan_pytorch_amd.metrics.official import OfficialMetrics
    name = 'a_96x128_noise8'
    true, pred = clip_pair(name)
    tt, pp = torch.from_numpy(true).to(DEV), torch.from_numpy(pred).to(DEV)
    n = true.shape[0] - 2 * CUTFR
    # the naive form: three forward() calls on the cropped frames
    t, p, (y, x, h, w) = _evaluated(name)
    tc, pc = t[:, y:y + h, x:x + w].contiguous(), p[:, y:y + h, x:x + w].contiguous()
    lp = lpips(tc, pc)
    tlp = (lpips(tc[:-1].contiguous(), tc[1:].contiguous()) - lpips(pc[:-1].contiguous(), pc[1:].contiguous())).abs() * 100.0
    frames = []
    real = ops.lpips_conv

    def counting(x0, wt, bias, cout, ks, stride, pad, x1=None, lut=None, out=None):
        if ks == 11:
            frames.append(x0.shape[0] + (0 if x1 is None else x1.shape[0]))
        return real(x0, wt, bias, cout, ks, stride, pad, x1=x1, lut=lut, out=out)
    monkeypatch.setattr(ops, 'lpips_conv', counting)
    for chunk in (1, 2, None):
        del frames[:]
        r = OfficialMetrics(lpips, device=DEV, chunk_frames=chunk).compute_sequence(tt, pp)
        assert r['LPIPS'] == lp.tolist() and r['tLP100'] == tlp.tolist(), chunk
        assert sum(frames) == 2 * n, (chunk, frames)          # conv1 ran once per frame and side
    del frames[:]
    r = OfficialMetrics(lpips, device=DEV, reuse_features=False).compute_sequence(tt, pp)
    assert r['LPIPS'] == lp.tolist() and r['tLP100'] == tlp.tolist() and sum(frames) == 2 * n + 4 * (n - 1)
    assert len(r['tLP100']) == n - 1 == 2


def _check_against_folder_golden(doc, g):
    assert doc['skipped'] == ['tOF'] and doc['keys'] == ['PSNR', 'SSIM', 'LPIPS', 'tLP100']
    eps32 = 2.0 ** -23
    for k in ('PSNR', 'SSIM'):           # values equal upstream's to ~1e-13 before the float32 casts
        for key in ('FrameAvg_', 'FolderAvg_'):
            assert abs(doc[key + k] - float(g['agg_' + key + k])) <= 4 * eps32 * abs(doc[key + k]), key + k
        assert np.all(np.abs(np.array(doc['Avg_' + k]) - g['agg_Avg_' + k]) <= 4 * eps32 * g['agg_Avg_' + k])
    lp = np.concatenate([g[f'{n}_lpips64'] for n in FOLDER_CASES])
    assert abs(doc['FrameAvg_LPIPS'] - lp.mean()) <= b(lp).mean() + eps32 * lp.mean()
    assert abs(doc['FrameAvg_LPIPS'] - float(g['agg_FrameAvg_LPIPS'])) <= 2 * b(lp).mean()
    tb = np.concatenate([100.0 * (b(g[f'{n}_dgt64']) + b(g[f'{n}_dout64'])) for n in FOLDER_CASES])
    tl = np.concatenate([g[f'{n}_tlp64'] for n in FOLDER_CASES])
    assert abs(doc['FrameAvg_tLP100'] - tl.mean()) <= tb.mean() + eps32 * tl.mean()
    assert doc['frame_counts'] == {'PSNR': 5, 'SSIM': 5, 'LPIPS': 5, 'tLP100': 3}


def test_cli_end_to_end(tmp_path, lpips, golden):
    from tecogan_pytorch_amd.metrics.official import OfficialMetrics
    g = golden('official')
    torch.save(alexnet_state_dict(), str(tmp_path / 'alexnet.pth'))
    torch.save(_lin_sd(golden), str(tmp_path / 'alex.pth'))
    res, tar = [], []
    for name in FOLDER_CASES:
        true, pred = clip_pair(name)
        tar.append(write_folder(tmp_path, f'gt_{name}', true))
        res.append(write_folder(tmp_path, f'sr_{name}', pred))
    doc = OfficialMetrics(lpips, device=DEV).evaluate_folders(res, tar, str(tmp_path / 'inproc'), quiet=True)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    out = subprocess.run([sys.executable, '-m', 'tecogan_pytorch_amd.metrics.official', '--results', ','.join(res),
                          '--targets', ','.join(tar), '--output', str(tmp_path / 'cli'), '--alexnet',
                          str(tmp_path / 'alexnet.pth'), '--lin', str(tmp_path / 'alex.pth')],
                         env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    cli = json.load(open(tmp_path / 'cli' / 'metrics.json'))
    assert cli == json.loads(json.dumps(doc))                 # bit for bit, a fresh process
    assert 'PSNR, total frame 5, total avg' in out.stdout and out.stdout.rstrip().endswith('Finished.')
    assert (tmp_path / 'cli' / 'metricsfile.txt').read_text() == (tmp_path / 'inproc' / 'metricsfile.txt').read_text()
    _check_against_folder_golden(cli, g)
    for f, name in zip(cli['folders'], FOLDER_CASES):
        assert np.all(np.abs(np.array(f['SSIM']) - g[f'{name}_ssim']) <= 1e-9)
        assert np.all(np.abs(np.array(f['LPIPS']) - g[f'{name}_lpips64']) <= b(g[f'{name}_lpips64']))


def test_mode_test_official_hook(tmp_path, lpips, golden):
    """`test.official_metrics: true`: {name}_official.json equals compute_sequence on the frames save_res wrote;
    the in-loop JSON is still written."""
    import yaml
    from PIL import Image
    from procedural_weights import generator_state_dict, smooth_clip
    from tecogan_pytorch_amd import main as M
    from tecogan_pytorch_amd.metrics.official import OfficialMetrics, aggregate, folder_sums
    torch.save(generator_state_dict(scale=4, degradation='BD'), str(tmp_path / 'G_iter30.pth'))
    torch.save(alexnet_state_dict(), str(tmp_path / 'alexnet.pth'))
    torch.save(_lin_sd(golden), str(tmp_path / 'alex.pth'))
    seqs, nfr = {}, {'calendar': 6, 'city': 7}
    for i, (key, t) in enumerate(nfr.items()):
        gt = (smooth_clip(t, 3, 128, 160, seed=60 + i).permute(0, 2, 3, 1) * 255).round().clamp(0, 255)
        seqs[key] = gt.to(torch.uint8).numpy()
        for f in range(t):
            path = tmp_path / 'GT' / key / f'{f:08d}.png'
            path.parent.mkdir(parents=True, exist_ok=True)
            Image.fromarray(seqs[key][f]).save(str(path))
    opt = M.default_opt()
    opt['model']['name'] = 'FRVSR'
    opt['model']['generator']['load_path'] = str(tmp_path / 'G_iter30.pth')
    opt['dataset']['test'] = {'name': 'Vid4', 'gt_seq_dir': str(tmp_path / 'GT'), 'lr_seq_dir': None}
    opt['test'].update({'save_res': True, 'res_dir': str(tmp_path / 'res'), 'save_json': True,
                        'json_dir': str(tmp_path / 'json'), 'num_pad_front': 2, 'official_metrics': True})
    opt['metric'] = {'PSNR': {'colorspace': 'y'},
                     'LPIPS': {'model': 'net-lin', 'net': 'alex', 'colorspace': 'rgb', 'spatial': False, 'version': 0.1,
                               'net_path': str(tmp_path / 'alexnet.pth'), 'lin_path': str(tmp_path / 'alex.pth')}}
    (tmp_path / 'test.yml').write_text(yaml.safe_dump(opt, sort_keys=False))
    M.main(['--mode', 'test', '--exp_dir', str(tmp_path), '--opt', 'test.yml'])
    assert list(json.load(open(tmp_path / 'json' / 'Vid4_avg.json'))['G_iter30']) == ['PSNR', 'LPIPS']
    got = json.load(open(tmp_path / 'json' / 'Vid4_official.json'))
    om = OfficialMetrics(lpips, device=DEV)
    exp = {}
    for key, t in nfr.items():
        saved = np.stack([np.asarray(Image.open(tmp_path / 'res' / 'Vid4' / 'G_iter30' / key / f'{f:08d}.png'))
                          for f in range(t)])
        exp[key] = om.compute_sequence(seqs[key], saved)
    assert got['sequences'] == ['calendar', 'city'] and got['skipped'] == ['tOF'] and got['model'] == 'G_iter30'
    assert got['frames'] == [6, 7] and got['evaluated'] == [2, 3] and got['windows'] == [exp[k]['window'] for k in nfr]
    for key in nfr:
        assert got['per_frame'][key] == {k: exp[key][k] for k in om.keys}, key
    agg = json.loads(json.dumps(aggregate([folder_sums(exp[k]) for k in nfr])))
    for k, v in agg.items():
        assert got[k] == v, k
    assert 5.0 < got['FrameAvg_PSNR'] < 60.0 and 0.0 < got['FrameAvg_SSIM'] <= 1.0 and got['FrameAvg_LPIPS'] > 0.0
