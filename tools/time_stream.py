#!/usr/bin/env python3
"""FRNet.infer_stream against FRNet.infer_sequence, and a long run.  The profiler is off; every time
is a host clock around work that ends in a synchronisation.  Needs a GPU: there is no fallback.

1. rate: a 60-frame HOST clip at 3x134x320 (4x BD, fp32) through infer_stream (fed frame by frame, every chunk copied
   out of its ring slot) and through infer_sequence(host clip, pipeline=True) -- the path that existed before the stream
   and that the stream leaves untouched.  Both are warmed, then --repeats regions of each alternate in ONE process (as
   tools/time_fp16.py does); medians, min-max of each, and their ratio are recorded.
2. long: --long-frames frames of the same size produced chunk by chunk from a seed and never held as a whole; frames/s
   over the first and the last 1000 frames, the peak device memory (which must equal that of a 120-frame stream), and
   the plan's fault / re-arm counters at the end.

    python tools/time_stream.py [--repeats 7] [--long-frames 6000] [--out profiles/stream_inference.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

C, H, W, SCALE, DEG = 3, 134, 320, 4, 'BD'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=60)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--long-frames', type=int, default=6000)
    ap.add_argument('--out', type=str, default=os.path.join(ROOT, 'profiles', 'stream_inference.json'))
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error('--repeats must be at least 5')
    import torch
    if not torch.cuda.is_available():
        sys.exit('time_stream.py: an MI355X is required (no fallback)')
    from tecogan_pytorch_amd.models.networks import FRNet
    from tecogan_pytorch_amd.models.networks.tecogan_nets import STREAM_SLOTS, stream_batch_sizes
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    net = FRNet(C, C, 64, 10, DEG, SCALE).to(dev).eval()
    gen = torch.Generator(device='cpu').manual_seed(1234)
    clip = torch.rand(args.steps, C, H, W, generator=gen)           # on the host

    def run_sequence():
        out = net.infer_sequence(clip, dev, pipeline=True)           # (synchronises; pinned host array)
        return out.shape[0]

    def run_stream(frames=None):
        n = 0
        for chunk in net.infer_stream((f for f in clip) if frames is None else frames, dev):
            n += chunk.copy().shape[0]                               # what a caller that keeps the frames pays
        torch.cuda.synchronize()
        return n

    result = {'protocol': 'host clip / host frames in, uint8 frames on the host out; profiler off; host clock around '
                          'regions that end in a synchronisation; the two paths alternate in one process',
              'lr_size': f'{C}x{H}x{W}', 'scale': SCALE, 'degradation': DEG, 'precision': 'fp32',
              'device': torch.cuda.get_device_name(0), 'stream_slots': STREAM_SLOTS,
              'batch_sizes_first_later': list(stream_batch_sizes())}

    # -- 1. rate against the existing path ------------------------------------------------------------------------------
    for _ in range(2):
        assert run_sequence() == args.steps and run_stream() == args.steps
    net.check_faults()
    times = {'infer_sequence': [], 'infer_stream': []}
    for _ in range(args.repeats):
        for name, fn in (('infer_sequence', run_sequence), ('infer_stream', run_stream)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
            net.check_faults()
    fps = {m: sorted(args.steps / t for t in ts) for m, ts in times.items()}
    med = {m: statistics.median(v) for m, v in fps.items()}
    spread = fps['infer_sequence'][-1] - fps['infer_sequence'][0]
    rate = {'frames': args.steps, 'repeats': args.repeats, 'fps_median': med,
            'fps_min': {m: v[0] for m, v in fps.items()}, 'fps_max': {m: v[-1] for m, v in fps.items()}, 'fps_all': fps,
            'infer_sequence_spread_fps': spread, 'ratio_stream_over_sequence': med['infer_stream'] / med['infer_sequence'],
            'stream_median_inside_sequence_min_max': bool(fps['infer_sequence'][0] <= med['infer_stream'] <= fps['infer_sequence'][-1]),
            'stream_median_below_sequence_median_by_more_than_its_spread':
                bool(med['infer_sequence'] - med['infer_stream'] > spread)}
    result['rate'] = rate
    print(json.dumps(rate), flush=True)

    # -- 2. a long run --------------------------------------------------------------------------------------------------
    def produced(total, seed, chunk=16):
        """Chunks of a clip that never exists as a whole: one seeded base chunk, shifted by a seeded offset per chunk
        (a host copy of 8 MB -- cheap enough not to be what is measured, unlike 2 M random numbers per chunk)."""
        g = torch.Generator(device='cpu').manual_seed(seed)
        base = torch.rand(chunk, C, H, W, generator=g)
        left = total
        while left:
            m = min(left, chunk)
            shift = int(torch.randint(0, W, (1,), generator=g))
            yield torch.roll(base, shifts=shift, dims=3)[:m]
            left -= m

    def peak_of(total, marks=None):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        n, t0 = 0, time.perf_counter()
        for chunk in net.infer_stream(produced(total, 99), dev):
            n += len(chunk)
            if marks is not None:
                marks.append((n, time.perf_counter() - t0))
        torch.cuda.synchronize()
        assert n == total
        return torch.cuda.max_memory_allocated()

    def span_fps(marks, lo, hi):
        """frames/s between the first chunk boundary at or after frame lo and the last one at or before frame hi."""
        inside = [(n, t) for n, t in marks if lo <= n <= hi]
        (n0, t0), (n1, t1) = inside[0], inside[-1]
        return (n1 - n0) / (t1 - t0), n1 - n0

    peak_120 = peak_of(120)
    marks = []
    peak_long = peak_of(args.long_frames, marks)
    net.check_faults()
    plan = net._get_plan(1, H, W, dev)
    faults, active = plan.chain_state()
    rearms, wait = plan.rearm_state()
    first, n_first = span_fps(marks, 0, 1000)
    last, n_last = span_fps(marks, args.long_frames - 1000, args.long_frames)
    long_run = {'frames': args.long_frames, 'produced_in_chunks_of': 16,
                'fps_first_1000': first, 'fps_last_1000': last, 'frames_in_those_spans': [n_first, n_last],
                'fps_whole': args.long_frames / marks[-1][1],
                'note': 'the producer (a shifted host copy of a seeded 16-frame chunk, same thread) is inside these times',
                'peak_device_bytes': peak_long, 'peak_device_bytes_120_frames': peak_120,
                'peak_equals_120_frame_stream': bool(peak_long == peak_120),
                'chain_faults': faults, 'one_launch_body_in_use': active, 'rearms': rearms, 'rearm_wait_frames': wait}
    result['long_run'] = long_run
    print(json.dumps(long_run), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
    print('wrote', args.out)
    if peak_long != peak_120:
        sys.exit('time_stream.py: the peak of the long stream differs from that of a 120-frame stream')


if __name__ == '__main__':
    main()
