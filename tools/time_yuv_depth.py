#!/usr/bin/env python3
"""What 10- and 12-bit YUV 4:2:0 costs the stream.  The protocol is tools/time_yuv.py's: a 60-frame
HOST clip at 3x134x320 (4x BD, fp32), every form warmed, --repeats alternating regions of each in ONE process, profiler
off, host clock around regions that end in a synchronisation; medians and min-max.  Needs a GPU: there is no fallback.

1. stream: FRNet.infer_stream(yuv=...) fed frames one by one, every chunk copied out of its ring slot, in three forms:
   8-bit in and out (section 7e's path, which the new fields leave untouched), 8 -> 10 (the same input, the output
   written from the float HR frame: one launch behind EVERY frame in place of one per batch) and 10 -> 10.
2. converter: tg_rgb_f32_to_yuv420p16 alone, n = 1 at the HR size, against a device copy that moves the same bytes
   (half of read + written each way), --launches launches back to back between two device events; nobody has
   measured it before, so it is reported and nothing is asserted.
3. untouched (with --parent-root DIR, a built checkout of the parent commit): the uint8 RGB stream of
   tools/time_yuv.py on this tree and on the parent's, in child processes that alternate (each imports the package of
   the tree it is given, warms up, and times --child-regions regions).  Acceptance is section 7d's rule: the new median
   lies inside the parent's min-max.

    python tools/time_yuv_depth.py [--repeats 7] [--parent-root DIR] [--out profiles/yuv_depth.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C, H, W, SCALE, DEG = 3, 134, 320, 4, 'BD'


def fps_summary(times, frames):
    fps = {m: sorted(frames / t for t in ts) for m, ts in times.items()}
    return {'frames': frames, 'repeats': {m: len(v) for m, v in fps.items()},
            'fps_median': {m: statistics.median(v) for m, v in fps.items()}, 'fps_min': {m: v[0] for m, v in fps.items()},
            'fps_max': {m: v[-1] for m, v in fps.items()}, 'fps_all': fps}


def alternate(forms, repeats, sync):
    times = {name: [] for name, _ in forms}
    for _ in range(repeats):
        for name, fn in forms:
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            times[name].append(time.perf_counter() - t0)
    return times


def make_net(root):
    sys.path.insert(0, root)
    import torch
    if not torch.cuda.is_available():
        sys.exit('time_yuv_depth.py: an MI355X is required (no fallback)')
    from tecogan_pytorch_amd import main as M
    from tecogan_pytorch_amd.models import define_model
    torch.manual_seed(0)
    opt = M.default_opt()
    opt.update({'is_train': False, 'dist': False, 'device': 'cuda', 'rank': 0, 'world_size': 1})
    return define_model(opt).net_G.eval()


def child(root, steps, regions):
    """The untouched uint8 RGB stream on the tree at `root`: prints one JSON line with the seconds of every region."""
    import numpy as np
    import torch
    net = make_net(root)
    import tecogan_pytorch_amd
    assert os.path.dirname(os.path.abspath(tecogan_pytorch_amd.__file__)).startswith(os.path.abspath(root)), 'wrong tree'
    dev = torch.device('cuda', 0)
    rgb_clip = np.random.default_rng(1234).integers(0, 256, (steps, H, W, C), dtype=np.uint8)

    def run_rgb():
        n = 0
        for chunk in net.infer_stream((f for f in rgb_clip), dev):
            n += chunk.copy().shape[0]
        assert n == steps
    for _ in range(2):
        run_rgb()
    net.check_faults()
    times = alternate((('rgb_u8', run_rgb),), regions, torch.cuda.synchronize)
    net.check_faults()
    print('CHILD ' + json.dumps(times['rgb_u8']), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=60)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--parent-root', dest='parent_root', type=str, default=None)
    ap.add_argument('--child-rounds', dest='child_rounds', type=int, default=3)
    ap.add_argument('--child-regions', dest='child_regions', type=int, default=5)
    ap.add_argument('--child', type=str, default=None, help=argparse.SUPPRESS)
    ap.add_argument('--out', type=str, default=os.path.join(HERE, 'profiles', 'yuv_depth.json'))
    args = ap.parse_args()
    if args.child is not None:
        return child(args.child, args.steps, args.child_regions)
    if args.repeats < 5:
        ap.error('--repeats must be at least 5')
    import numpy as np
    net = make_net(HERE)
    import torch
    from tecogan_pytorch_amd import _lib as L, ops
    from tecogan_pytorch_amd.models.networks import Yuv420
    from tecogan_pytorch_amd.models.networks.tecogan_nets import STREAM_SLOTS, stream_batch_sizes
    dev = torch.device('cuda', 0)
    sync = torch.cuda.synchronize
    rng = np.random.default_rng(1234)
    specs = {'yuv_8_8': Yuv420(H, W), 'yuv_8_10': Yuv420(H, W, out_depth=10), 'yuv_10_10': Yuv420(H, W, depth=10)}
    clips = {'yuv_8_8': rng.integers(0, 256, (args.steps, specs['yuv_8_8'].frame_bytes), dtype=np.uint8)}
    clips['yuv_8_10'] = clips['yuv_8_8']
    clips['yuv_10_10'] = rng.integers(0, 1024, (args.steps, specs['yuv_10_10'].frame_bytes // 2), dtype=np.uint16).view(np.uint8)

    def runner(name):
        def run():
            n = 0
            for chunk in net.infer_stream((f for f in clips[name]), dev, yuv=specs[name]):
                n += chunk.copy().shape[0]
            assert n == args.steps
        return run
    result = {'protocol': 'host frames in one by one, every chunk copied out of its ring slot; profiler off; host clock '
                          'around regions that end in a synchronisation; the forms alternate in one process',
              'lr_size': f'{C}x{H}x{W}', 'scale': SCALE, 'degradation': DEG, 'precision': 'fp32',
              'device': torch.cuda.get_device_name(0), 'stream_slots': STREAM_SLOTS,
              'batch_sizes_first_later': list(stream_batch_sizes()),
              'bytes_per_lr_frame': {k: s.frame_bytes for k, s in specs.items()},
              'bytes_per_hr_frame': {k: s.out_frame_bytes(SCALE) for k, s in specs.items()}}

    # -- 1. the stream ---------------------------------------------------------------------------------------------------
    forms = tuple((name, runner(name)) for name in specs)
    for _ in range(2):
        for _, fn in forms:
            fn()
    net.check_faults()
    result['stream'] = fps_summary(alternate(forms, args.repeats, sync), args.steps)
    net.check_faults()
    med = result['stream']['fps_median']
    result['stream']['ms_per_frame_over_yuv_8_8'] = {k: 1e3 / med[k] - 1e3 / med['yuv_8_8'] for k in med}
    print(json.dumps(result['stream']), flush=True)

    # -- 2. the converter alone ------------------------------------------------------------------------------------------
    HH, WW = SCALE * H, SCALE * W
    hr = torch.rand(1, 3, HH, WW, device=dev)
    out = torch.empty(1, HH * WW * 3 // 2, dtype=torch.uint16, device=dev)
    read_b, write_b = hr.numel() * 4, out.numel() * 2
    half = (read_b + write_b) // 2
    a, b = torch.empty(half, dtype=torch.uint8, device=dev), torch.empty(half, dtype=torch.uint8, device=dev)
    lib, st = L.lib(), torch.cuda.current_stream().cuda_stream
    codes = specs['yuv_8_10'].codes()

    def convert():
        L.check(lib.tg_rgb_f32_to_yuv420p16(hr.data_ptr(), out.data_ptr(), 1, HH, WW, 10, *codes, st), 'convert')

    def timed(fn):
        for _ in range(20):
            fn()
        sync()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.launches):
            fn()
        e1.record()
        sync()
        return e0.elapsed_time(e1) * 1e3 / args.launches            # microseconds per launch
    us = {'convert': [], 'copy': []}
    for _ in range(args.repeats):
        us['convert'].append(timed(convert))
        us['copy'].append(timed(lambda: b.copy_(a)))
    assert torch.equal(out, ops.rgb_f32_to_yuv420p(hr, 10, *specs['yuv_8_10'].codes()))
    cm, pm = statistics.median(us['convert']), statistics.median(us['copy'])
    result['converter'] = {'size': f'{HH}x{WW}', 'bytes_read': read_b, 'bytes_written': write_b, 'copy_bytes_each_way': half,
                           'launches_per_region': args.launches, 'us_per_launch_all': us,
                           'us_per_launch_median': {'convert': cm, 'copy': pm},
                           'gb_per_s': {'convert': (read_b + write_b) / cm / 1e3, 'copy': 2 * half / pm / 1e3},
                           'ratio_convert_over_copy': cm / pm,
                           'note': 'back-to-back launches between two device events: launch overhead included, the '
                                   'input stays in the cache hierarchy between launches'}
    print(json.dumps(result['converter']), flush=True)

    # -- 3. the untouched RGB path, this tree against the parent's ----------------------------------------------------------
    if args.parent_root:
        roots = {'parent': os.path.abspath(args.parent_root), 'this': HERE}
        secs = {k: [] for k in roots}
        del net
        torch.cuda.empty_cache()
        for _ in range(args.child_rounds):
            for k, root in roots.items():
                r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', root, '--steps', str(args.steps),
                                    '--child-regions', str(args.child_regions)], capture_output=True, text=True,
                                   timeout=300, env=dict(os.environ, PYTHONPATH=root))
                line = [ln for ln in r.stdout.splitlines() if ln.startswith('CHILD ')]
                if r.returncode != 0 or not line:
                    sys.exit('time_yuv_depth.py: the %s child failed (%d): %s' % (k, r.returncode, r.stderr[-2000:]))
                secs[k] += json.loads(line[0][6:])
        un = fps_summary(secs, args.steps)
        un['protocol'] = ('%d child processes per tree, alternating parent / this, each warmed and timing %d regions of '
                          'the uint8 RGB stream' % (args.child_rounds, args.child_regions))
        un['this_median_inside_parent_min_max'] = bool(un['fps_min']['parent'] <= un['fps_median']['this'] <= un['fps_max']['parent'])
        un['ratio_this_over_parent'] = un['fps_median']['this'] / un['fps_median']['parent']
        result['untouched_rgb_stream'] = un
        print(json.dumps(un), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
