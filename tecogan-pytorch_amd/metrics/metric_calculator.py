"""MetricCalculator with the reference's API and semantics (codes/metrics/metric_calculator.py:16-226):
per-frame metric lists per sequence, frames cropped to the smaller of the two sizes, sequence
means, a cross-rank sum to rank 0, averages, display and the JSON file of `save`.

On the HIP path: PSNR (`y` / `rgb`) is compute_psnr_device (exact squared-error sums on the device),
LPIPS is metrics/lpips.py (alex / net-lin / v0.1, spatial false).  Sequences may be device tensors or
numpy arrays ((t,h,w,3) uint8); numpy inputs are uploaded.  tOF (:222-279) is computed only when its section
says `backend: hip`: ops.tof, Farneback's flow as DESIGN.md section 7f restates it (not compared with OpenCV), on
the whole size-matched frames, first frame skipped.  Any other tOF section is announced once and left out of the
results, as OpenCV's flow is not part of this port."""
import json
import logging
import os.path as osp
from collections import OrderedDict

import numpy as np
import torch

from ..utils import dist_utils
from .lpips import LPIPS
from .psnr import compute_psnr_device

log = logging.getLogger('tecogan_pytorch_amd')


def validate_lpips_cfg(cfg):
    cfg = cfg or {}
    if cfg.get('model', 'net-lin') != 'net-lin':
        raise ValueError(f"LPIPS: model {cfg.get('model')!r} is not supported (net-lin only)")
    if cfg.get('net', 'alex') != 'alex':
        raise ValueError(f"LPIPS: net {cfg.get('net')!r} is not supported (alex only)")
    if str(cfg.get('version', '0.1')) != '0.1':
        raise ValueError(f"LPIPS: version {cfg.get('version')!r} is not supported (0.1 only)")
    if cfg.get('spatial', False):
        raise ValueError('LPIPS: spatial: true is not supported (per-frame scalars only)')


def _model_order(item):
    """The reference sorts models by the iteration in `G_iter<k>`; other names follow, by name."""
    k = item[0].replace('G_iter', '')
    return (0, int(k), '') if k.isdigit() else (1, 0, item[0])


class MetricCalculator:
    def __init__(self, opt, lpips=None):
        """opt: the run's options (`metric`, `device`, `dist`, `rank`).  lpips: an LPIPS instance to
        use instead of loading the weights the `LPIPS` section names."""
        self.metric_opt = OrderedDict()
        for mtype, cfg in opt['metric'].items():
            if mtype == 'tOF' and (cfg or {}).get('backend') == 'hip':
                self.metric_opt[mtype] = cfg
                continue
            if mtype == 'tOF':
                log.warning('metric tOF (OpenCV Farneback optical flow) is not available here; it is left out')
                continue
            if mtype not in ('PSNR', 'LPIPS'):
                raise ValueError(f'Unrecognized metric: {mtype} (PSNR | LPIPS | tOF)')
            self.metric_opt[mtype] = cfg or {}
        self.device = torch.device(opt.get('device', 'cuda'))
        self.dist = opt.get('dist', False)
        self.rank = opt.get('rank', 0)
        self.psnr_colorspace = ''
        self.lpips = None
        for mtype, cfg in self.metric_opt.items():
            if mtype == 'PSNR':
                self.psnr_colorspace = cfg.get('colorspace', 'y')
                if self.psnr_colorspace not in ('y', 'rgb'):
                    raise ValueError(f'PSNR: colorspace {self.psnr_colorspace!r} (y | rgb)')
            if mtype == 'LPIPS':
                validate_lpips_cfg(cfg)
                self.lpips = lpips if lpips is not None else LPIPS.from_config(cfg, device=self.device)
        self.reset()

    def reset(self):
        self.metric_dict = OrderedDict()
        self.avg_metric_dict = OrderedDict()

    def _upload(self, seq):
        if isinstance(seq, np.ndarray):
            seq = torch.from_numpy(np.ascontiguousarray(seq))
        if seq.dtype != torch.uint8 or seq.dim() != 4 or seq.shape[3] != 3:
            raise ValueError(f'expected (t,h,w,3) uint8 frames, got {seq.dtype} {tuple(seq.shape)}')
        return seq.to(self.device)

    def compute_sequence_metrics(self, seq_idx, true_seq, pred_seq):
        """Per-frame metrics of one sequence (thwc uint8, rgb) into metric_dict[seq_idx]."""
        true_seq, pred_seq = self._upload(true_seq), self._upload(pred_seq)
        if true_seq.shape[0] != pred_seq.shape[0]:
            raise ValueError(f'{seq_idx}: {true_seq.shape[0]} GT frames but {pred_seq.shape[0]} predicted')
        # pred and true may have different sizes: crop both to the smaller one (:184-191)
        h = min(true_seq.shape[1], pred_seq.shape[1])
        w = min(true_seq.shape[2], pred_seq.shape[2])
        true_seq = true_seq[:, :h, :w].contiguous()
        pred_seq = pred_seq[:, :h, :w].contiguous()
        md = self.metric_dict[seq_idx] = OrderedDict((m, []) for m in self.metric_opt)
        for mtype in self.metric_opt:
            if mtype == 'PSNR':
                md['PSNR'] = [float(v) for v in compute_psnr_device(true_seq, pred_seq, self.psnr_colorspace)]
            elif mtype == 'LPIPS':
                md['LPIPS'] = self.lpips(true_seq, pred_seq).tolist()
            elif mtype == 'tOF' and true_seq.shape[0] > 1:
                from .. import ops
                md['tOF'] = ops.tof(true_seq, pred_seq).tolist()

    def gather(self, seq_idx_lst):
        """Sequence means, summed over ranks into avg_metric_dict on rank 0 (:68-117)."""
        mtypes = list(self.metric_opt)
        vals = np.zeros((len(seq_idx_lst), len(mtypes)), dtype=np.float64)
        for s, seq_idx in enumerate(seq_idx_lst):
            if seq_idx in self.metric_dict:
                for i, m in enumerate(mtypes):
                    vals[s, i] = np.mean(self.metric_dict[seq_idx][m])
        dev = self.device if (self.dist and self.device.type == 'cuda') else 'cpu'
        red = dist_utils.reduce_sum_to_master(vals.reshape(-1).tolist(), device=dev).cpu().numpy()
        red = red.reshape(len(seq_idx_lst), len(mtypes))
        if self.rank == 0:
            for s, seq_idx in enumerate(seq_idx_lst):
                self.avg_metric_dict[seq_idx] = OrderedDict((m, float(red[s, i])) for i, m in enumerate(mtypes))

    def average(self):
        out = OrderedDict()
        for m in self.metric_opt:
            out[m] = np.mean([d[m] for d in self.avg_metric_dict.values()])
        return out

    @dist_utils.master_only
    def display(self):
        for seq_idx, d in self.avg_metric_dict.items():
            print(f'Sequence: {seq_idx}')
            for m in self.metric_opt:
                print(f'\t{m}: {d[m]:.6f}')
        print('Average')
        for m, v in self.average().items():
            print(f'\t{m}: {v:.6f}')

    @dist_utils.master_only
    def save(self, model_idx, save_path, average=True, override=False):
        """{model_idx: {metric: '%.6f'}} merged into save_path, models sorted by iteration (:139-172)."""
        if osp.exists(save_path):
            with open(save_path, 'r') as f:
                json_dict = json.load(f)
        else:
            json_dict = dict()
        if model_idx not in json_dict:
            json_dict[model_idx] = OrderedDict()
        if not average:
            raise NotImplementedError('per-sequence results are not saved (as in the reference)')
        for m, v in self.average().items():
            if m in json_dict[model_idx] and not override:
                continue
            json_dict[model_idx][m] = f'{v:.6f}'
        json_dict = OrderedDict(sorted(json_dict.items(), key=_model_order))
        with open(save_path, 'w') as f:
            json.dump(json_dict, f, sort_keys=False, indent=4)
