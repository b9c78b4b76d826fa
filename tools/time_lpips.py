#!/usr/bin/env python
"""LPIPS (alex / net-lin / v0.1) on one 576 x 720 frame pair: ms per pair and per stage, HIP events.

    python tools/time_lpips.py [--h 576 --w 720 --pairs 1 --reps 50]

Weights are seeded fan-in-uniform (timing does not depend on their values).  conv1 / conv2 report
their share of the fp32 MFMA peak (157.3 TFLOP/s, MI355X spec): algorithmic FLOP (2 * cout * K *
output pixels) over event time.  Events bracket each stage in isolation, so the per-stage numbers
include one launch each; `total` is one whole forward()."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_F32 = 157.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--h', type=int, default=576)
    ap.add_argument('--w', type=int, default=720)
    ap.add_argument('--pairs', type=int, default=1)
    ap.add_argument('--reps', type=int, default=50)
    a = ap.parse_args()
    import tecogan_pytorch_amd  # noqa: F401
    from tecogan_pytorch_amd import ops
    from tecogan_pytorch_amd.metrics.lpips import ALEX_CONVS, CHNS, LPIPS, alexnet_out_sizes
    assert torch.cuda.is_available(), 'time_lpips needs a GPU'
    g = torch.Generator().manual_seed(0)
    sd = {}
    for idx, ci, co, k, _, _ in ALEX_CONVS:
        b = 1.4 / (ci * k * k) ** 0.5
        sd[f'features.{idx}.weight'] = (torch.rand(co, ci, k, k, generator=g) * 2 - 1) * b * 3 ** 0.5
        sd[f'features.{idx}.bias'] = (torch.rand(co, generator=g) * 2 - 1) * b
    lin = {f'lin{k}.model.1.weight': torch.rand(1, c, 1, 1, generator=g) * 0.1 for k, c in enumerate(CHNS)}
    m = LPIPS('cuda')
    m.load_alexnet_state_dict(sd)
    m.load_lin_state_dict(lin)
    t = a.pairs
    x = torch.randint(0, 256, (t, a.h, a.w, 3), generator=g, dtype=torch.uint8).cuda()
    y = torch.randint(0, 256, (t, a.h, a.w, 3), generator=g, dtype=torch.uint8).cuda()
    packed, lins, lut = m._device_weights()
    sizes = alexnet_out_sizes(a.h, a.w)
    n = 2 * t
    # stage inputs, produced once
    c1 = ops.lpips_conv(x, packed[0][0], packed[0][1], 64, 11, 4, 2, x1=y, lut=lut)
    p1 = ops.maxpool3s2(c1)
    c2 = ops.lpips_conv(p1, packed[1][0], packed[1][1], 192, 5, 1, 2)
    p2 = ops.maxpool3s2(c2)
    feats = m.features(x, y)
    res = torch.zeros(t, 5, device='cuda')
    tot = torch.zeros(t, device='cuda')

    def conv3(i, src):
        wpk, b, ocb, cin, cout = packed[2 + i]
        out = torch.empty(n, cout, src.shape[2], src.shape[3], device='cuda')
        for j in range(n):
            ops.conv3x3(src[j:j + 1], wpk, b, cin, cout, ocb, act=ops.ACT_RELU, out=out[j:j + 1], ksplit=1)
    stages = {
        'conv1': (lambda: ops.lpips_conv(x, packed[0][0], packed[0][1], 64, 11, 4, 2, x1=y, lut=lut, out=c1),
                  2.0 * n * 64 * 363 * sizes[0][0] * sizes[0][1]),
        'pool1': (lambda: ops.maxpool3s2(c1, out=p1), 0),
        'conv2': (lambda: ops.lpips_conv(p1, packed[1][0], packed[1][1], 192, 5, 1, 2, out=c2),
                  2.0 * n * 192 * 1600 * sizes[1][0] * sizes[1][1]),
        'pool2': (lambda: ops.maxpool3s2(c2, out=p2), 0),
        'conv3': (lambda: conv3(0, p2), 2.0 * n * 384 * 192 * 9 * sizes[2][0] * sizes[2][1]),
        'conv4': (lambda: conv3(1, feats[2]), 2.0 * n * 256 * 384 * 9 * sizes[2][0] * sizes[2][1]),
        'conv5': (lambda: conv3(2, feats[3]), 2.0 * n * 256 * 256 * 9 * sizes[2][0] * sizes[2][1]),
        'heads': (lambda: [ops.lpips_head(f[:t], f[t:], lins[k], res, k, tot if k == 4 else None)
                           for k, f in enumerate(feats)], 0),
        'total': (lambda: m(x, y), 0),
    }
    out = {'h': a.h, 'w': a.w, 'pairs': t, 'reps': a.reps, 'ms_per_pair': {}}
    for name, (fn, flop) in stages.items():
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / a.reps
        out['ms_per_pair'][name] = round(ms / t, 4)
        if flop:
            out[f'{name}_tflops'] = round(flop / (ms * 1e-3) / 1e12, 2)
            out[f'{name}_frac_f32_mfma_peak'] = round(flop / (ms * 1e-3) / PEAK_F32, 3)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
