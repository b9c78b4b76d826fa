#!/usr/bin/env python
"""The official protocol's metrics on the device: ms per 576 x 720 frame pair for SSIM (tg_ssim_y_u8) and float-Y
PSNR (tg_psnr_yfloat_sse_u8) on the crop_8x8 window, and for a clip the whole OfficialMetrics.compute_sequence
with and without feature reuse.  HIP events, warm-up, median of --reps repeats (>= 11).

    python tools/time_official_metrics.py [--h 576 --w 720 --frames 20 --reps 11]

Weights are seeded fan-in-uniform (timing does not depend on their values).  compute_sequence includes its host
work (the PSNR partials and the per-frame lists come back to the host), as a caller sees it."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_ms(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--h', type=int, default=576)
    ap.add_argument('--w', type=int, default=720)
    ap.add_argument('--frames', type=int, default=20)
    ap.add_argument('--reps', type=int, default=11)
    a = ap.parse_args()
    assert a.reps >= 11, 'median of at least 11 repeats'
    import tecogan_pytorch_amd  # noqa: F401
    from tecogan_pytorch_amd import ops
    from tecogan_pytorch_amd.metrics.lpips import ALEX_CONVS, CHNS, LPIPS
    from tecogan_pytorch_amd.metrics.official import OfficialMetrics, crop_8x8_window
    assert torch.cuda.is_available(), 'time_official_metrics needs a GPU'
    g = torch.Generator().manual_seed(0)
    sd = {}
    for idx, ci, co, k, _, _ in ALEX_CONVS:
        b = 1.4 / (ci * k * k) ** 0.5
        sd[f'features.{idx}.weight'] = (torch.rand(co, ci, k, k, generator=g) * 2 - 1) * b * 3 ** 0.5
        sd[f'features.{idx}.bias'] = (torch.rand(co, generator=g) * 2 - 1) * b
    lin = {f'lin{k}.model.1.weight': torch.rand(1, c, 1, 1, generator=g) * 0.1 for k, c in enumerate(CHNS)}
    m = LPIPS('cuda', scaling=True)
    m.load_alexnet_state_dict(sd)
    m.load_lin_state_dict(lin)
    t = a.frames
    x = torch.randint(0, 256, (t, a.h, a.w, 3), generator=g, dtype=torch.uint8).cuda()
    y = torch.randint(0, 256, (t, a.h, a.w, 3), generator=g, dtype=torch.uint8).cuda()
    win = crop_8x8_window(a.h, a.w)
    out = {'h': a.h, 'w': a.w, 'window': list(win), 'frames': t, 'reps': a.reps}
    med, lo, hi = median_ms(lambda: ops.ssim_y_u8(x, y, win), a.reps)
    out['ssim_ms_per_pair'] = {'median': round(med / t, 4), 'min': round(lo / t, 4), 'max': round(hi / t, 4)}
    med, lo, hi = median_ms(lambda: ops.ssim_y_u8(x[:1], y[:1], win), a.reps)
    out['ssim_ms_one_pair_per_call'] = {'median': round(med, 4), 'min': round(lo, 4), 'max': round(hi, 4)}
    med, lo, hi = median_ms(lambda: ops.psnr_yfloat_sse_u8(x, y, win), a.reps)
    out['psnr_yfloat_ms_per_pair'] = {'median': round(med / t, 4), 'min': round(lo / t, 4), 'max': round(hi / t, 4)}
    for reuse in (True, False):
        om = OfficialMetrics(m, cutfr=2, reuse_features=reuse)
        med, lo, hi = median_ms(lambda: om.compute_sequence(x, y), a.reps, warmup=2)
        out['sequence_ms_' + ('reuse' if reuse else 'naive')] = {'median': round(med, 2), 'min': round(lo, 2),
                                                                 'max': round(hi, 2)}
    out['evaluated_frames'] = t - 4
    print(json.dumps(out))


if __name__ == '__main__':
    main()
