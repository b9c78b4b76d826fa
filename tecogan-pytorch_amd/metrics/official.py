"""The official TecoGAN evaluation protocol (codes/official_metrics/metrics.py, evaluate.py), device-resident:
the numbers of the published benchmark table, as opposed to the in-loop MetricCalculator.

Per folder pair (results, targets), frames [cutfr, n - cutfr) only, temporal metrics from the second of those on:
  * both frames are cropped at the top left to the smaller of the two sizes, then `crop_8x8` takes a centred
    window whose sides are multiples of 32 and which removes at least 8 pixels per side;
  * PSNR on the UNROUNDED Y plane (tg_psnr_yfloat_sse_u8: exact integer sums; identical frames give inf);
  * SSIM on the same Y planes (tg_ssim_y_u8: 7x7 uniform window, data_range of the predicted frame);
  * LPIPS alex / net-lin / v0.1 WITH ScalingLayer (DistModel's default is the string '0.1'; `--mode test`
    follows the ymls, whose float 0.1 skips it);
  * tLP100 = |LPIPS(out[i-1], out[i]) - LPIPS(gt[i-1], gt[i])| * 100 in fp32.  The AlexNet taps of a frame are
    computed once (LPIPS.features_of) and serve the three head evaluations it takes part in;
  * three averages with the script's float32 casts: Avg_<k> per folder, FolderAvg_<k>, FrameAvg_<k>.
Both crops are window arguments of the kernels; only LPIPS reads a contiguous copy of the window.

tOF is opt-in (tof=True, --tof, test.official_tof): Farneback flows of consecutive target and result frames
(ops.tof; both on the size-matched, otherwise uncropped frames, crop_8x8 applied to the flows), computed by the HIP
restatement of the algorithm that DESIGN.md section 7f specifies.  It has not been compared with OpenCV, which the
JSON says under "tOF_flow".  Without the opt-in tOF is listed under "skipped", as before.
Not reproduced: metrics.csv (pandas' print format).  A folder with at most 2 * cutfr frames has empty lists; its
averages are nan as numpy's 0 / 0 is in the script, and it is listed under "empty_folders".

CLI:  python -m tecogan_pytorch_amd.metrics.official --results a,b --targets c,d --output dir [--alexnet P --lin P]
      python -m tecogan_pytorch_amd.metrics.official --model TecoGAN_BD [--data_root data --results_root results]
      --tof adds the tOF column."""
import argparse
import json
import math
import os
import os.path as osp
from collections import OrderedDict

import numpy as np
import torch

KEYS = ('PSNR', 'SSIM', 'LPIPS', 'tLP100')
SKIPPED = ('tOF',)
KEYS_TOF = ('PSNR', 'SSIM', 'LPIPS', 'tOF', 'tLP100')     # the script's order, with tOF switched on
TOF_FLOW_NOTE = 'farneback, restated, not compared with OpenCV'
EVAL_SETS = (('Vid4', ('calendar', 'city', 'foliage', 'walk')), ('ToS3', ('bridge', 'face', 'room')))


def crop_8x8_window(h, w):
    """(y, x, ch, cw) of crop_8x8 (metrics.py:75-90): sides floored to multiples of 32, reduced by 32 until at
    least 16 pixels are removed, centred."""
    ch, cw = (h // 32) * 32, (w // 32) * 32
    while ch > h - 16:
        ch -= 32
    while cw > w - 16:
        cw -= 32
    return (h - ch) // 2, (w - cw) // 2, ch, cw


def list_png(dirpath):
    """listPNGinDir (metrics.py:27-34): *.png only, names starting with IB skipped, sorted by name and then
    (stably) by the integer made of all the digits of the name (-1 without digits)."""
    names = [n for n in os.listdir(dirpath) if n.endswith('.png') and not n.startswith('IB')]
    names.sort()
    names.sort(key=lambda n: int(''.join(c for c in n if c.isdigit()) or -1))
    return [osp.join(dirpath, n) for n in names]


def folder_sums(lists, keys=KEYS):
    """{key: (float32 sum, count)} of one folder's per-frame lists: all the aggregates need (np.float32(list).sum())."""
    return OrderedDict((k, (np.float32(lists[k]).sum(dtype=np.float32), len(lists[k]))) for k in keys)


def aggregate(sums, keys=KEYS):
    """The script's three averages (metrics.py:193-226) from per-folder (float32 sum, count) pairs, in folder
    order, in its float32 arithmetic: Avg_<k> (list), FolderAvg_<k>, FrameAvg_<k>, and frame_counts."""
    out = OrderedDict()
    counts = OrderedDict()
    with np.errstate(invalid='ignore', divide='ignore'):
        for k in keys:
            tot, folder, n, avg = np.float32(0), np.float32(0), 0, []
            for s in sums:
                v, c = np.float32(s[k][0]), int(s[k][1])
                mean = v / np.float32(c)
                avg.append(float(mean))
                tot = np.float32(tot + v)
                folder = np.float32(folder + mean)
                n += c
            out['Avg_' + k] = avg
            out['FolderAvg_' + k] = float(folder / np.float32(len(sums))) if sums else float('nan')
            out['FrameAvg_' + k] = float(tot / np.float32(n))
            counts[k] = n
    out['frame_counts'] = counts
    return out


def summary_lines(agg, keys=KEYS):
    return ['%s, total frame %d, total avg %02.4f, folder avg %02.4f' %
            (k, agg['frame_counts'][k], agg['FrameAvg_' + k], agg['FolderAvg_' + k]) for k in keys]


class OfficialMetrics:
    """lpips: an LPIPS instance built with scaling=True (None: PSNR and SSIM only; LPIPS and tLP100 are then
    listed under "skipped").  chunk_frames bounds the frames whose AlexNet taps are alive at once (None: the
    LPIPS instance's own rule); no value depends on it.  reuse_features=False evaluates the three LPIPS terms
    with three forward() calls (six backbone passes per frame): the same values, for timing and tests.
    tof=True adds tOF in the script's position (PSNR, SSIM, LPIPS, tOF, tLP100; PSNR, SSIM, tOF without lpips)."""

    def __init__(self, lpips=None, device='cuda', cutfr=2, chunk_frames=None, reuse_features=True, tof=False):
        if lpips is not None and not lpips.scaling:
            raise ValueError('OfficialMetrics: the official protocol runs LPIPS with ScalingLayer (scaling=True)')
        self.lpips = lpips
        self.device = torch.device(device)
        self.cutfr = int(cutfr)
        self.chunk_frames = chunk_frames
        self.reuse_features = reuse_features
        self.tof = bool(tof)
        self.keys = KEYS if lpips is not None else KEYS[:2]
        self.skipped = list(SKIPPED) + [k for k in KEYS if k not in self.keys]
        if self.tof:
            self.keys = tuple(k for k in KEYS_TOF if k == 'tOF' or k in self.keys)
            self.skipped = [k for k in KEYS if k not in self.keys]

    @classmethod
    def from_paths(cls, alexnet=None, lin=None, device='cuda', **kw):
        """Weight paths resolve as in LPIPS.from_config (argument, environment, torchvision's cache)."""
        from .lpips import LPIPS
        cfg = {'net_path': alexnet, 'lin_path': lin, 'version': '0.1'}
        return cls(LPIPS.from_config(cfg, device=device, scaling=True), device=device, **kw)

    crop_8x8_window = staticmethod(crop_8x8_window)

    def _upload(self, seq):
        if isinstance(seq, np.ndarray):
            seq = torch.from_numpy(np.ascontiguousarray(seq))
        if seq.dtype != torch.uint8 or seq.dim() != 4 or seq.shape[3] != 3:
            raise ValueError(f'expected (t,h,w,3) uint8 frames, got {seq.dtype} {tuple(seq.shape)}')
        return seq.to(self.device).contiguous()

    def frame_range(self, n_target, n_result):
        """The frames the script reads: range(cutfr, n_target - cutfr); the results must reach that far."""
        lo, hi = self.cutfr, n_target - self.cutfr
        if hi > lo and n_result < hi:
            raise ValueError(f'{n_target} target frames need results up to frame {hi - 1}, got {n_result}')
        return lo, max(lo, hi)

    def window(self, true_hw, pred_hw):
        h, w = min(true_hw[0], pred_hw[0]), min(true_hw[1], pred_hw[1])
        y, x, ch, cw = crop_8x8_window(h, w)
        if ch < 7 or cw < 7 or (self.lpips is not None and (ch < 31 or cw < 31)):
            raise ValueError(f'frames of {h}x{w} crop to {ch}x{cw}: too small for '
                             f'{"LPIPS (31x31)" if ch >= 7 and cw >= 7 else "SSIM (7x7)"}')
        if self.tof and (h < 16 or w < 16):
            raise ValueError(f'frames of {h}x{w}: too small for tOF (16x16)')
        return y, x, ch, cw

    def _lpips_terms(self, tc, pc):
        """LPIPS(gt[i], out[i]) for every frame and tLP100 from the second on: fp32 device tensors."""
        m = self.lpips
        n = tc.shape[0]
        if not self.reuse_features:
            lp = m(tc, pc)
            if n < 2:
                return lp, lp.new_zeros(0)
            return lp, (m(tc[:-1], tc[1:]) - m(pc[:-1], pc[1:])).abs() * 100.0
        step = max(1, int(self.chunk_frames)) if self.chunk_frames else max(1, m._chunk(n, tc.shape[1], tc.shape[2]))
        lp, tlp, prev = [], [], None
        for f0 in range(0, n, step):
            ft, fp = m.features_of(tc[f0:f0 + step]), m.features_of(pc[f0:f0 + step])
            lp.append(m.distance(ft, fp))
            if prev is not None:          # the pair that straddles two chunks: the last frame's taps are kept
                tlp.append((m.distance(prev[0], [f[:1] for f in ft]) -
                            m.distance(prev[1], [f[:1] for f in fp])).abs() * 100.0)
            if ft[0].shape[0] > 1:
                tlp.append((m.distance([f[:-1] for f in ft], [f[1:] for f in ft]) -
                            m.distance([f[:-1] for f in fp], [f[1:] for f in fp])).abs() * 100.0)
            prev = ([f[-1:] for f in ft], [f[-1:] for f in fp])
        return torch.cat(lp), (torch.cat(tlp) if tlp else lp[0].new_zeros(0))

    def compute_sequence(self, true_seq, pred_seq):
        """(t,h,w,3) uint8 frames (device tensors or numpy) of one folder pair -> per-frame lists PSNR, SSIM,
        LPIPS (t - 2 cutfr values), tOF (with tof=True) and tLP100 (one fewer), plus 'frames' (t), 'evaluated' and
        'window'
        (y, x, h, w; None when no frame is evaluated)."""
        lo, hi = self.frame_range(true_seq.shape[0], pred_seq.shape[0])
        out = self.compute_frames(true_seq[lo:hi], pred_seq[lo:hi])
        out['frames'] = int(true_seq.shape[0])
        return out

    def compute_frames(self, true_seq, pred_seq):
        """compute_sequence on frames that are already the protocol's range: every frame is evaluated."""
        from .. import ops
        out = OrderedDict((k, []) for k in self.keys)
        out.update(frames=int(true_seq.shape[0]), evaluated=int(true_seq.shape[0]), window=None)
        if true_seq.shape[0] == 0:
            return out
        t, p = self._upload(true_seq), self._upload(pred_seq)
        if t.shape[0] != p.shape[0]:
            raise ValueError(f'{t.shape[0]} target frames, {p.shape[0]} results')
        win = self.window(t.shape[1:3], p.shape[1:3])
        y, x, h, w = win
        out['window'] = list(win)
        ssim = ops.ssim_y_u8(t, p, win)
        sse = ops.psnr_yfloat_sse_u8(t, p, win)
        for s in sse:                     # 20 log10(255 / sqrt(mean((Y_true - Y_pred)^2))), Y = 16 + y' / 255000
            out['PSNR'].append(float('inf') if s == 0 else
                               float(20.0 * np.log10(255.0 / math.sqrt(s / (255000.0 ** 2 * h * w)))))
        out['SSIM'] = ssim.tolist()
        if self.lpips is not None:
            tc, pc = t[:, y:y + h, x:x + w].contiguous(), p[:, y:y + h, x:x + w].contiguous()
            lp, tlp = self._lpips_terms(tc, pc)
            out['LPIPS'], out['tLP100'] = lp.tolist(), tlp.tolist()
        if self.tof and t.shape[0] > 1:   # flows on the size-matched, uncropped frames; crop_8x8 on the flows
            out['tOF'] = ops.tof(t, p, win).tolist()
        return out

    def evaluate_folders(self, result_dirs, target_dirs, output_dir, quiet=False):
        """The whole script for lists of result / target folders: metrics.json, metricsfile.txt (appended)."""
        from ..data.folder_dataset import read_rgb
        if len(result_dirs) != len(target_dirs) or not result_dirs:
            raise ValueError(f'{len(result_dirs)} result folders for {len(target_dirs)} target folders')
        os.makedirs(output_dir, exist_ok=True)
        folders, sums, empty = [], [], []
        for rdir, tdir in zip(result_dirs, target_dirs):
            res, tar = list_png(rdir), list_png(tdir)
            lo, hi = self.frame_range(len(tar), len(res))
            if hi > lo:                   # frames outside [lo, hi) are never decoded
                r = self.compute_frames(np.stack([read_rgb(f) for f in tar[lo:hi]]),
                                        np.stack([read_rgb(f) for f in res[lo:hi]]))
            else:
                r = self.compute_frames(np.zeros((0, 1, 1, 3), np.uint8), np.zeros((0, 1, 1, 3), np.uint8))
                empty.append(len(folders))
            r['frames'] = len(tar)
            folders.append(OrderedDict([('result', rdir), ('target', tdir)] + list(r.items())))
            sums.append(folder_sums(r, self.keys))
        doc = OrderedDict(keys=list(self.keys), skipped=self.skipped, cutfr=self.cutfr, folders=folders,
                          empty_folders=empty)
        if self.tof:
            doc['tOF_flow'] = TOF_FLOW_NOTE
        doc.update(aggregate(sums, self.keys))
        lines = summary_lines(doc, self.keys)
        with open(osp.join(output_dir, 'metricsfile.txt'), 'a') as f:
            f.write('\n'.join(lines) + '\n')
        if not quiet:
            print('\n'.join(lines))
        with open(osp.join(output_dir, 'metrics.json'), 'w') as f:
            json.dump(doc, f, indent=2)
        return doc


def reduce_and_aggregate(per_seq, seq_ids, keys, device='cpu'):
    """`--mode test`: per_seq {seq_idx: compute_sequence result} of THIS rank -> the aggregates over all ranks'
    sequences in seq_ids order on rank 0.  Ranks exchange per-sequence float32 sums and counts only (each sequence
    is non-zero on exactly one rank; float32 values pass through the float64 reduction unchanged)."""
    from ..utils import dist_utils
    vals = np.zeros((len(seq_ids), len(keys), 2), dtype=np.float64)
    for i, sid in enumerate(seq_ids):
        if sid in per_seq:
            for j, (v, c) in enumerate(folder_sums(per_seq[sid], keys).values()):
                vals[i, j] = (float(v), c)
    red = dist_utils.reduce_sum_to_master(vals.reshape(-1).tolist(), device=device).cpu().numpy()
    red = red.reshape(vals.shape)
    sums = [OrderedDict((k, (np.float32(red[i, j, 0]), int(red[i, j, 1]))) for j, k in enumerate(keys))
            for i in range(len(seq_ids))]
    return aggregate(sums, keys)


def main(argv=None):
    ap = argparse.ArgumentParser(description='official TecoGAN metrics (PSNR, SSIM, LPIPS, tLP100) on the GPU')
    ap.add_argument('--results', help='comma-separated result folders')
    ap.add_argument('--targets', help='comma-separated target folders')
    ap.add_argument('--output', help='output directory (metrics.json, metricsfile.txt)')
    ap.add_argument('--model', '-m', help='e.g. TecoGAN_BD: evaluate results_root/{Vid4,ToS3}/<model> as evaluate.py')
    ap.add_argument('--data_root', default='data')
    ap.add_argument('--results_root', default='results')
    ap.add_argument('--alexnet', help='torchvision alexnet state dict')
    ap.add_argument('--lin', help="the v0.1 alex linear-layer weights (alex.pth)")
    ap.add_argument('--device', default='cuda')
    ap.add_argument('--tof', action='store_true', help='add tOF (Farneback flow as DESIGN.md 7f restates it; '
                                                       'not compared with OpenCV)')
    args = ap.parse_args(argv)
    jobs = []
    if args.model:
        keys = args.model.split('_')
        if len(keys) < 2 or keys[0] not in ('TecoGAN', 'FRVSR') or keys[1] not in ('BD', 'BI'):
            ap.error(f'--model {args.model}: expected (TecoGAN|FRVSR)_(BD|BI)')
        for name, vids in EVAL_SETS:
            sr = osp.join(args.results_root, name, args.model)
            if osp.exists(sr):
                jobs.append(([osp.join(sr, v) for v in vids],
                             [osp.join(args.data_root, name, 'GT', v) for v in vids], osp.join(sr, 'metric_log')))
    elif args.results and args.targets and args.output:
        jobs.append((args.results.split(','), args.targets.split(','), args.output))
    else:
        ap.error('give --results, --targets and --output, or --model')
    if not jobs:
        print(f'no result folder of {args.model} under {args.results_root}')
        return []
    om = OfficialMetrics.from_paths(args.alexnet, args.lin, device=args.device, tof=args.tof)
    docs = [om.evaluate_folders(*job) for job in jobs]
    print('Finished.')
    return docs


if __name__ == '__main__':
    main()
