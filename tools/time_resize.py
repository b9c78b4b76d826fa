#!/usr/bin/env python3
"""What the resize to any size costs on the GPU.  The protocol is tools/time_png.py's (its
helpers are imported): a 60-frame HOST clip at 3x134x320 (4x BD, fp32, HR 536x1280), every form warmed, --repeats
alternating regions of each in ONE process, profiler off; medians, min-max and the ratio.  Needs a GPU: there is no
fallback.

1. call: ops.resize_u8 alone on 8 HR frames of 536x1280 -> 402x960 (3/4) and -> 268x640 (1/2), regions of --launches
   launches between device events, against tg_copy_ceiling moving the same bytes ((in + out) / 2 read and written) with
   the kernel's own grid.
2. stream: FRNet.infer_stream(resize=Resize(402, 960)) fed uint8 RGB frames one by one, every chunk copied, against
   FRNet.infer_stream without it; host clock around regions that end in a synchronisation.
3. untouched: --baseline-only (with --root, a checkout of another commit) times infer_stream WITHOUT resize alone and
   writes its record; --untouched PARENT NEW PARENT NEW takes four such records (one job, that order) and applies
   DESIGN.md section 7d's rule.  --bench takes `name=frames/s` figures of bench.py from the same job.

    python tools/time_resize.py [--repeats 7] [--launches 20] [--out profiles/resize.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from time_png import alternate, summary, untouched_rule     # noqa: E402

C, H, W, SCALE, DEG = 3, 134, 320, 4, 'BD'
CALL_FRAMES = 8
SIZES = [(402, 960), (268, 640)]
STREAM_SIZE = SIZES[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=60)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--root', type=str, default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help='the checkout whose package is measured')
    ap.add_argument('--baseline-only', action='store_true', help='infer_stream without resize alone (any commit)')
    ap.add_argument('--untouched', nargs=4, metavar='JSON', default=None,
                    help='four --baseline-only records of one job: parent, new, parent, new')
    ap.add_argument('--bench', nargs='*', metavar='NAME=FPS', default=[], help="bench.py's figures of the same job")
    ap.add_argument('--out', type=str, default=None)
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error('--repeats must be at least 5')
    sys.path.insert(0, os.path.abspath(args.root))
    out_path = args.out or os.path.join(os.path.abspath(args.root), 'profiles', 'resize.json')
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit('time_resize.py: an MI355X is required (no fallback)')
    from tecogan_pytorch_amd import main as M
    from tecogan_pytorch_amd.models import define_model
    from tecogan_pytorch_amd.models.networks.tecogan_nets import STREAM_SLOTS, stream_batch_sizes
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    opt = M.default_opt()
    opt.update({'is_train': False, 'dist': False, 'device': 'cuda', 'rank': 0, 'world_size': 1})
    net = define_model(opt).net_G.eval()
    rng = np.random.default_rng(1234)
    rgb_clip = rng.integers(0, 256, (args.steps, H, W, C), dtype=np.uint8)
    sync = torch.cuda.synchronize

    def run_stream(**kw):
        def run():
            n = 0
            for chunk in net.infer_stream((f for f in rgb_clip), dev, **kw):
                n += chunk.copy().shape[0]
            assert n == args.steps
        return run

    run_rgb = run_stream()
    result = {'protocol': 'host frames in one by one, every chunk copied out of its ring slot; profiler off; host clock '
                          'around regions that end in a synchronisation; the two forms alternate in one process',
              'lr_size': f'{C}x{H}x{W}', 'scale': SCALE, 'degradation': DEG, 'precision': 'fp32',
              'device': torch.cuda.get_device_name(0), 'stream_slots': STREAM_SLOTS,
              'batch_sizes_first_later': list(stream_batch_sizes())}

    if args.baseline_only:
        for _ in range(2):
            run_rgb()
        times = alternate((('rgb_u8', run_rgb),), args.repeats, sync)
        net.check_faults()
        fps = sorted(args.steps / t for t in times['rgb_u8'])
        result['untouched_stream'] = {'frames': args.steps, 'repeats': args.repeats, 'fps_median': statistics.median(fps),
                                      'fps_min': fps[0], 'fps_max': fps[-1], 'fps_all': fps}
        print(json.dumps(result['untouched_stream']), flush=True)
        with open(out_path, 'w') as f:
            json.dump(result, f, indent=1)
        print('wrote', out_path)
        return

    from tecogan_pytorch_amd import _lib as L, ops
    from tecogan_pytorch_amd.models.networks import Resize

    # -- 1. the call alone -------------------------------------------------------------------------------------------------
    HR = (SCALE * H, SCALE * W)
    x = torch.from_numpy(rng.integers(0, 256, (CALL_FRAMES,) + HR + (3,), dtype=np.uint8)).to(dev)
    lib = L.lib()

    def region(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        sync()
        a.record()
        for _ in range(args.launches):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / args.launches              # microseconds per call

    result['call'] = {'protocol': 'regions of %d launches between device events, the two forms alternating, '
                                  'microseconds per call' % args.launches, 'frames': CALL_FRAMES, 'from': list(HR)}
    for size in SIZES:
        y = torch.empty(CALL_FRAMES, *size, 3, dtype=torch.uint8, device=dev)
        nbytes = x.numel() + y.numel()
        half = (nbytes // 2 + 15) // 16 * 16
        src = torch.empty(half, dtype=torch.uint8, device=dev).random_(0, 256)
        dst = torch.empty_like(src)
        blocks = CALL_FRAMES * -(-size[0] // 8) * -(-size[1] // 32)  # the resize kernel's grid: tiles of 8 x 32 pixels

        def resize(y=y, size=size):
            ops.resize_u8(x, size, out=y)

        def copy(src=src, dst=dst, half=half, blocks=blocks):
            L.check(lib.tg_copy_ceiling(src.data_ptr(), dst.data_ptr(), half, blocks, 256, ops._stream()), 'tg_copy_ceiling')
        forms = (('resize', resize), ('copy_same_bytes', copy))
        for _, fn in forms:
            for _ in range(3):
                fn()
        times = {name: [] for name, _ in forms}
        for _ in range(args.repeats):
            for name, fn in forms:
                times[name].append(region(fn))
        rec = {name: {'us_median': statistics.median(v), 'us_min': min(v), 'us_max': max(v), 'us_all': v}
               for name, v in times.items()}
        rec['bytes'] = {'in': x.numel(), 'out': y.numel()}
        rec['resize_GBps_of_compulsory_bytes'] = nbytes / rec['resize']['us_median'] * 1e-3
        rec['resize_fraction_of_copy'] = rec['copy_same_bytes']['us_median'] / rec['resize']['us_median']
        rec['us_per_frame'] = rec['resize']['us_median'] / CALL_FRAMES
        result['call']['to_%dx%d' % size] = rec
        print(json.dumps({('to_%dx%d' % size): {k: v for k, v in rec.items() if not isinstance(v, dict) or k == 'bytes'}}),
              flush=True)

    # -- 2. the stream ---------------------------------------------------------------------------------------------------
    run_resized = run_stream(resize=Resize(*STREAM_SIZE))
    for _ in range(2):
        run_rgb()
        run_resized()
    net.check_faults()
    times = alternate((('rgb_u8', run_rgb), ('resized', run_resized)), args.repeats, sync)
    net.check_faults()
    result['stream'] = summary(times, args.steps, 'resized', 'rgb_u8')
    result['stream']['resized_to'] = list(STREAM_SIZE)
    med = result['stream']['fps_median']
    result['stream']['ms_per_batch_of_%d_added' % stream_batch_sizes()[1]] = \
        (1.0 / med['resized'] - 1.0 / med['rgb_u8']) * 1e3 * stream_batch_sizes()[1]
    print(json.dumps(result['stream']), flush=True)

    # -- 3. the untouched path ---------------------------------------------------------------------------------------------
    if args.untouched:
        recs = []
        for p in args.untouched:
            with open(p) as f:
                recs.append(json.load(f)['untouched_stream'])
        result['untouched_stream'] = untouched_rule(recs)
        print(json.dumps({k: v for k, v in result['untouched_stream'].items() if k not in ('parent', 'new')}), flush=True)
    if args.bench:
        result['bench_py_frames_per_s'] = {k: float(v) for k, v in (b.split('=') for b in args.bench)}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'w') as f:
        json.dump(result, f, indent=1)
    print('wrote', out_path)


if __name__ == '__main__':
    main()
