#!/usr/bin/env python3
"""fp32 against fp16 clip inference, measured alternately in ONE process.

The headline's protocol (bench.py): FRNet.infer_sequence on a device-resident K-frame clip, uint8 frames left on
the device, one timed region = exactly K steps between synchronisations.  At each configuration both modes are
warmed (plans, buffers, event rings), then fp32 and fp16 regions alternate `--repeats` times (at least five); the
medians, the min-max spread of each mode, their ratio and the uint8 / PSNR distance between the two modes' frames
go to a JSON under profiles/.  Needs a GPU: there is no fallback.

    python tools/time_fp16.py [--steps 60] [--warmup 8] [--repeats 7] [--out profiles/fp16_inference.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = [('3x134x320', 4, 'BD'), ('3x268x640', 2, 'BI')]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=60)
    ap.add_argument('--warmup', type=int, default=8)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--out', type=str, default=os.path.join(ROOT, 'profiles', 'fp16_inference.json'))
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error('--repeats must be at least 5')
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit('time_fp16.py: an MI355X is required (no fallback)')
    from tecogan_pytorch_amd import _lib as L
    from tecogan_pytorch_amd.models.networks import FRNet
    dev = torch.device('cuda', 0)
    result = {'protocol': 'FRNet.infer_sequence, device-resident clip, uint8 on device, pipelined flow passes; '
                          'fp32 / fp16 regions alternate in one process, profiler off',
              'steps': args.steps, 'warmup': args.warmup, 'repeats': args.repeats,
              'device': torch.cuda.get_device_name(0), 'configs': []}
    for lr_size, s, deg in CONFIGS:
        c, h, w = [int(v) for v in lr_size.split('x')]
        torch.manual_seed(0)
        nets = {'fp32': FRNet(c, c, 64, 10, deg, s).to(dev).eval()}
        nets['fp16'] = FRNet(c, c, 64, 10, deg, s, precision='fp16').to(dev).eval()
        nets['fp16'].load_state_dict(nets['fp32'].state_dict(), strict=True)
        gen = torch.Generator(device='cpu').manual_seed(1234)
        clip = torch.rand(args.steps, c, h, w, generator=gen).to(dev)
        wclip = torch.rand(max(args.warmup, 2), c, h, w, generator=gen).to(dev)
        frames = {}
        with torch.no_grad():
            for mode, net in nets.items():
                net.infer_sequence(wclip, dev, return_device_tensor=True)
                torch.cuda.synchronize()
                frames[mode] = net.infer_sequence(clip, dev, return_device_tensor=True).cpu().numpy()
                torch.cuda.synchronize()
                net.check_faults()
            times = {'fp32': [], 'fp16': []}
            for _ in range(args.repeats):
                for mode in ('fp32', 'fp16'):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    out = nets[mode].infer_sequence(clip, dev, return_device_tensor=True)
                    torch.cuda.synchronize()
                    times[mode].append(time.perf_counter() - t0)
                    nets[mode].check_faults()
                    del out
        fps = {m: sorted(args.steps / t for t in ts) for m, ts in times.items()}
        med = {m: statistics.median(v) for m, v in fps.items()}
        spread32 = fps['fp32'][-1] - fps['fp32'][0]
        d = np.abs(frames['fp32'].astype(np.int32) - frames['fp16'].astype(np.int32))
        mse = float((d.astype(np.float64) ** 2).mean())
        plan = nets['fp16']._get_plan(1, h, w, dev)
        row = {'lr_size': lr_size, 'scale': s, 'degradation': deg,
               'fps_median': med, 'fps_min': {m: v[0] for m, v in fps.items()}, 'fps_max': {m: v[-1] for m, v in fps.items()},
               'fps_all': fps, 'fp32_spread_fps': spread32, 'ratio_fp16_over_fp32': med['fp16'] / med['fp32'],
               'faster_than_fp32_by_more_than_its_spread': bool(med['fp16'] - med['fp32'] > spread32),
               'ms_per_frame_median': {m: 1e3 / v for m, v in med.items()},
               'u8_share_differing': float((d > 0).mean()), 'u8_max_difference': int(d.max()),
               'psnr_fp16_vs_fp32_db': (float('inf') if mse == 0 else float(10 * np.log10(255.0 ** 2 / mse))),
               'fp16_plan_launches_per_frame': L.lib().tg_frnet_plan_launches(plan.handle)}
        result['configs'].append(row)
        print(json.dumps(row), flush=True)
        del nets, frames
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
