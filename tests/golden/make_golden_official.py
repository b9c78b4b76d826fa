#!/usr/bin/env python
"""Golden vectors of the official evaluation protocol (codes/official_metrics/metrics.py of the upstream
reference), produced on the CPU in the authoring container only.

metrics.py is a script: it parses flags and imports cv2 / pandas / skimage at the top, so it cannot be imported.
Its source is parsed with `ast`, and ONLY the function definitions _rgb2ycbcr, to_uint8, psnr, ssim, crop_8x8 and
listPNGinDir are executed, in a namespace that holds numpy and os: upstream's code runs, none of it is copied.

`compare_ssim` is the one piece that can come neither from upstream nor from its dependency (skimage is not
installed).  It is supplied here as a restatement in fp64 on scipy.ndimage.uniform_filter, which is what skimage
calls, with skimage's defaults: 7x7 window, sample covariance (49/48), K1 0.01, K2 0.03, mean over the map cropped
by 3 pixels per side.  NOBODY HAS COMPARED THIS WITH skimage ITSELF on this project's machines; the risk is limited
to the constants of a published formula.

LPIPS / tLP100 run upstream's official_metrics/LPIPSmodels (PNetLin alex, v0.1 lin weights, util.im2tensor's
`v / (255 / 2) - 1` scaling) behind the import stubs of _ref_import, AlexNet carrying the procedural weights of
lpips_fixture.alexnet_state_dict as in make_golden_lpips.py, frame by frame with the script's loop semantics, in
fp32 (what upstream computes) and in fp64.  LPIPSmodels/v0.1/alex.pth is byte-identical to the lin file lpips.npz
holds (asserted below), so the tests take the lin weights from there.

The aggregates of the two-folder case follow the script's float32 casts (np.float32(list).sum() / len, ...).

Output: tests/golden/official.npz (per-frame scalars only)"""
import ast
import copy
import os
import sys
import tempfile

import numpy as np
import torch
from scipy.ndimage import uniform_filter

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _ref_import  # noqa: E402
from lpips_fixture import alexnet_state_dict  # noqa: E402
from official_fixture import CASES, CUTFR, DECOY_NAMES, FOLDER_CASES, clip_pair, crc, frame_file_names  # noqa: E402
from make_golden_lpips import _AlexNet  # noqa: E402

OFFICIAL = os.path.join(_ref_import.REF_CODES, 'official_metrics')
WANTED = ('_rgb2ycbcr', 'to_uint8', 'psnr', 'ssim', 'crop_8x8', 'listPNGinDir')
KEYS = ('PSNR', 'SSIM', 'LPIPS', 'tLP100')


def compare_ssim(X, Y, data_range):
    """skimage.measure.compare_ssim(X, Y, data_range=...) with its defaults, restated (see the module docstring)."""
    X, Y = X.astype(np.float64), Y.astype(np.float64)
    win, K1, K2 = 7, 0.01, 0.03
    NP = win ** X.ndim
    cov_norm = NP / (NP - 1)
    ux, uy = uniform_filter(X, size=win), uniform_filter(Y, size=win)
    uxx, uyy, uxy = uniform_filter(X * X, size=win), uniform_filter(Y * Y, size=win), uniform_filter(X * Y, size=win)
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    C1, C2 = (K1 * data_range) ** 2, (K2 * data_range) ** 2
    S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))
    pad = (win - 1) // 2
    return S[pad:-pad, pad:-pad].mean()


def upstream_functions():
    tree = ast.parse(open(os.path.join(OFFICIAL, 'metrics.py')).read())
    defs = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in WANTED]
    assert sorted(d.name for d in defs) == sorted(WANTED)
    ns = {'np': np, 'os': os, 'compare_ssim': compare_ssim}
    exec(compile(ast.Module(body=defs, type_ignores=[]), 'metrics.py', 'exec'), ns)
    return ns


def upstream_lpips():
    """(PNetLin fp32, PNetLin fp64, util) of official_metrics/LPIPSmodels."""
    _ref_import.import_reference()
    sys.modules['torchvision.models'].alexnet = lambda pretrained=True: _AlexNet()
    sys.path.insert(0, OFFICIAL)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        from LPIPSmodels import networks_basic as networks, util
    n32 = networks.PNetLin(use_gpu=False, pnet_type='alex', use_dropout=True, spatial=False, version='0.1')
    lin_sd = torch.load(os.path.join(OFFICIAL, 'LPIPSmodels', 'v0.1', 'alex.pth'), map_location='cpu')
    n32.load_state_dict(lin_sd)
    n32.eval()
    n32.net[0].eval()
    have = np.load(os.path.join(HERE, 'lpips.npz'))
    for k in range(5):
        assert np.array_equal(have[f'lin{k}'], lin_sd[f'lin{k}.model.1.weight'].numpy())
    n64 = copy.deepcopy(n32).double()
    n64.net = [copy.deepcopy(n32.net[0]).double()]          # a plain list: nn.Module.double() does not reach it
    n64.shift, n64.scale = n32.shift.double(), n32.scale.double()
    return n32, n64, util


def im2tensor64(image, cent=1., factor=255. / 2.):
    """util.im2tensor without its cast to fp32."""
    return torch.from_numpy(np.ascontiguousarray((image / factor - cent)[:, :, :, np.newaxis].transpose((3, 2, 0, 1))))


def run_folder(up, nets, true, pred):
    """The script's loop over one folder pair, frames [cutfr, n - cutfr), without tOF."""
    n32, n64, util = nets
    r = {k: [] for k in ('PSNR', 'SSIM', 'LPIPS', 'tLP100', 'LPIPS64', 'tLP64', 'dgt32', 'dout32', 'dgt64', 'dout64',
                         'range')}
    pre = None
    for i in range(CUTFR, true.shape[0] - CUTFR):
        out_img, tar_img = pred[i], true[i]
        if tar_img.shape[0] < out_img.shape[0] or tar_img.shape[1] < out_img.shape[1]:
            out_img = out_img[:tar_img.shape[0], :tar_img.shape[1]]
        if tar_img.shape[0] > out_img.shape[0] or tar_img.shape[1] > out_img.shape[1]:
            tar_img = tar_img[:out_img.shape[0], :out_img.shape[1]]
        tar_img, ofy, ofx = up['crop_8x8'](tar_img)
        out_img, ofy, ofx = up['crop_8x8'](out_img)
        r['window'] = np.array([ofy, ofx, tar_img.shape[0], tar_img.shape[1]])
        with np.errstate(all='raise'):
            r['PSNR'].append(up['psnr'](tar_img, out_img))
            r['SSIM'].append(up['ssim'](tar_img, out_img))
        yp = up['_rgb2ycbcr'](up['to_uint8'](out_img, 0, 255), 255)[:, :, 0]
        r['range'].append(yp.max() - yp.min())
        cur = (util.im2tensor(tar_img), util.im2tensor(out_img), im2tensor64(tar_img), im2tensor64(out_img))
        with torch.no_grad():
            r['LPIPS'].append(n32.forward(cur[0], cur[1]).numpy().flatten()[0])
            r['LPIPS64'].append(n64.forward(cur[2], cur[3]).item())
            if pre is not None:
                d0, d1 = n32.forward(pre[0], cur[0]).numpy().flatten(), n32.forward(pre[1], cur[1]).numpy().flatten()
                r['tLP100'].append((np.absolute(d0 - d1) * 100.0)[0])
                e0, e1 = n64.forward(pre[2], cur[2]).item(), n64.forward(pre[3], cur[3]).item()
                r['tLP64'].append(abs(e0 - e1) * 100.0)
                r['dgt32'].append(d0[0]); r['dout32'].append(d1[0]); r['dgt64'].append(e0); r['dout64'].append(e1)
        pre = cur
    assert r['LPIPS'][0].dtype == np.float32 and (not r['tLP100'] or r['tLP100'][0].dtype == np.float32)
    assert np.all(np.isfinite(r['PSNR'])) and np.all(np.isfinite(r['SSIM'])) and min(r['range']) >= 50, r['range']
    return r


def aggregates(folders):
    """Avg_ / FolderAvg_ / FrameAvg_ with the script's float32 casts."""
    out = {}
    for k in KEYS:
        frame_sum, frame_len, folder_sum, avg = 0, 0, 0, []
        for r in folders:
            cur = np.float32(r[k])
            s, n = cur.sum(), cur.shape[0]
            mean = s / n
            avg.append(mean)
            frame_sum += s
            frame_len += n
            folder_sum += mean
        out['Avg_' + k] = np.float32(avg)
        out['FrameAvg_' + k] = np.float64(frame_sum / frame_len)
        out['FolderAvg_' + k] = np.float64(folder_sum / len(folders))
        out['count_' + k] = np.int64(frame_len)
        assert avg[0].dtype == np.float32 and (frame_sum / frame_len).dtype == np.float32
    return out


def main():
    torch.set_num_threads(8)
    up = upstream_functions()
    nets = upstream_lpips()
    d = {'cases': np.array(list(CASES)), 'cutfr': np.int64(CUTFR)}
    res = {}
    for name in CASES:
        true, pred = clip_pair(name)
        r = res[name] = run_folder(up, nets, true, pred)
        d[f'{name}_crc'] = np.array([crc(true), crc(pred)], dtype=np.uint64)
        d[f'{name}_shape'] = np.array([true.shape, pred.shape])
        d[f'{name}_window'] = r['window']
        for k, key in (('PSNR', 'psnr'), ('SSIM', 'ssim'), ('LPIPS', 'lpips32'), ('LPIPS64', 'lpips64'),
                       ('tLP100', 'tlp32'), ('tLP64', 'tlp64'), ('dgt32', 'dgt32'), ('dout32', 'dout32'),
                       ('dgt64', 'dgt64'), ('dout64', 'dout64'), ('range', 'range')):
            d[f'{name}_{key}'] = np.array(r[k], dtype=np.float64)
        print(name, 'window', r['window'], 'psnr', np.round(r['PSNR'], 3), 'ssim', np.round(r['SSIM'], 5))
        print('   lpips64', np.round(r['LPIPS64'], 5), 'tlp64', np.round(r['tLP64'], 5),
              'range', np.round(r['range'], 1))
        print('   fp32 rel err', np.max(np.abs(np.array(r['LPIPS'], dtype=np.float64) - r['LPIPS64']) /
                                        np.array(r['LPIPS64'])))
    for k, v in aggregates([res[n] for n in FOLDER_CASES]).items():
        d['agg_' + k] = v
        print('agg', k, v)
    # listPNGinDir on the folder case's file names plus decoys
    names = frame_file_names(CASES[FOLDER_CASES[1]][0])
    with tempfile.TemporaryDirectory() as tmp:
        for n in list(names) + list(DECOY_NAMES):
            open(os.path.join(tmp, n), 'w').close()
        got = [os.path.basename(p) for p in up['listPNGinDir'](tmp)]
    assert got == names, got
    d['listing_files'] = np.array(sorted(list(names) + list(DECOY_NAMES)))
    d['listing_order'] = np.array(got)
    path = os.path.join(HERE, 'official.npz')
    np.savez_compressed(path, **d)
    print('official.npz', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
