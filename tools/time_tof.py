#!/usr/bin/env python
"""What tOF costs: the official evaluator on a synthetic 41-frame 576 x 720 pair of sequences (Vid4's size and the
length of its shortest clip), with and without tof=True, both warmed, then --reps alternating regions per mode in one
process, profiler off; median and min-max.  Also the flow alone (ops.farneback_flow on one chunk) in ms per frame pair,
each stage's algorithmic bytes (what the stage must read and write once, computed from the shapes), and the numpy
specification's time per pair on this host for context.

    python tools/time_tof.py [--h 576 --w 720 --frames 41 --reps 7] [--out profiles/tof.json] [--no-spec]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/time_tof.py --trace   (flow only, one chunk)

With kernel times from such a trace, achieved bytes/s of a stage = its algorithmic bytes here / its kernel time."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stage_bytes(h, w, pairs, levels):
    """Algorithmic bytes per stage for `pairs` pairs (pairs + 1 frames): every input and output counted once."""
    f = pairs + 1
    out = {'fb_gray': f * h * w * 4}
    for k, (lh, lw) in enumerate(levels):
        n = lh * lw
        out.setdefault('fb_hblur', 0)
        out['fb_hblur'] += f * h * w * 5                                  # u8 in, fp32 out
        out.setdefault('fb_vblur_resize', 0)
        out['fb_vblur_resize'] += f * (h * w + n) * 4
        out.setdefault('fb_polyexp', 0)
        out['fb_polyexp'] += f * n * 6 * 4                                # 1 plane in, 5 out
        out.setdefault('fb_update', 0)
        out['fb_update'] += 3 * pairs * n * (10 + 2 + 5) * 4             # R0, R1, flow in; M out; 3 per level
        out.setdefault('fb_blur_solve', 0)
        out['fb_blur_solve'] += 3 * pairs * n * (5 + 2) * 4
        if k + 1 < len(levels):
            out.setdefault('fb_resize_flow', 0)
            out['fb_resize_flow'] += pairs * (n + levels[k + 1][0] * levels[k + 1][1]) * 8
    return out


def region_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(v, nd=2):
    return {'median': round(statistics.median(v), nd), 'min': round(min(v), nd), 'max': round(max(v), nd)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--h', type=int, default=576)
    ap.add_argument('--w', type=int, default=720)
    ap.add_argument('--frames', type=int, default=41)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--out', default=None)
    ap.add_argument('--no-spec', action='store_true', help='skip timing the numpy specification')
    ap.add_argument('--trace', action='store_true', help='flow of one chunk only, twice (for a kernel trace)')
    a = ap.parse_args()
    import tecogan_pytorch_amd  # noqa: F401
    from tecogan_pytorch_amd import ops
    from tecogan_pytorch_amd.metrics.official import OfficialMetrics
    from tests.farneback_fixture import sequence_pair
    from tests import farneback_ref as F
    assert torch.cuda.is_available(), 'time_tof needs a GPU'
    # a drifting texture and a noisy copy of it: flows with structure, as an evaluation has
    true, pred = sequence_pair(a.h, a.w, min(a.frames, 9), seed=0)
    reps = -(-a.frames // true.shape[0])
    true = np.concatenate([true, true[::-1]] * reps)[:a.frames]
    pred = np.concatenate([pred, pred[::-1]] * reps)[:a.frames]
    t, p = torch.from_numpy(true).cuda(), torch.from_numpy(pred).cuda()
    levels = ops.farneback_levels(a.h, a.w)
    chunk = 9
    if a.trace:
        for _ in range(2):
            ops.farneback_flow(t[:chunk])
        torch.cuda.synchronize()
        print(json.dumps({'traced': 'farneback_flow', 'pairs': chunk - 1, 'h': a.h, 'w': a.w,
                          'stage_bytes': stage_bytes(a.h, a.w, chunk - 1, levels)}))
        return
    out = {'h': a.h, 'w': a.w, 'frames': a.frames, 'reps': a.reps, 'levels': levels,
           'evaluated_frames': a.frames - 4, 'tof_pairs_per_sequence': a.frames - 5}
    plain, with_tof = OfficialMetrics(None, cutfr=2), OfficialMetrics(None, cutfr=2, tof=True)
    for om in (plain, with_tof, plain, with_tof):                          # warm both modes
        om.compute_sequence(t, p)
    ms = {'plain': [], 'tof': []}
    for _ in range(a.reps):                                                # alternating regions
        ms['plain'].append(region_ms(lambda: plain.compute_sequence(t, p)))
        ms['tof'].append(region_ms(lambda: with_tof.compute_sequence(t, p)))
    out['evaluator_ms_without_tof'] = stats(ms['plain'])
    out['evaluator_ms_with_tof'] = stats(ms['tof'])
    flows = 2 * (a.frames - 5)
    out['tof_ms_per_flow_in_evaluator'] = stats([(x - statistics.median(ms['plain'])) / flows for x in ms['tof']], 3)
    fl = [region_ms(lambda: ops.farneback_flow(t[:chunk])) / (chunk - 1) for _ in range(a.reps + 2)][2:]
    out['flow_ms_per_pair_chunk_of_%d' % chunk] = stats(fl, 3)
    out['stage_bytes_per_pair'] = {k: v // (chunk - 1) for k, v in stage_bytes(a.h, a.w, chunk - 1, levels).items()}
    out['launches_per_flow_call'] = 1 + len(levels) * 10
    if not a.no_spec:
        g0, g1 = F.gray_u8(true[0]), F.gray_u8(true[1])
        t0 = time.perf_counter()
        F.farneback(g0, g1)
        out['numpy_spec_s_per_pair'] = round(time.perf_counter() - t0, 2)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
