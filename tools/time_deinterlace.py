#!/usr/bin/env python3
"""What the deinterlacer costs.  The protocol is tools/time_yuv_planar.py's: every form warmed,
--repeats alternating regions of each in ONE process, profiler off; kernels between two device events, streams under the
host clock around regions that end in a synchronisation; medians and min-max.  Needs a GPU: there is no fallback.

a. the kernel alone: tg_deinterlace_planar, 8 frames (and the frame before) in, 16 out, at 576x720 4:2:0 8-bit and at
   1080x1920 4:2:2 10-bit, --launches launches back to back, against a device-to-device copy that moves the bytes it
   reads plus writes (about two frames read and one written per output frame: half of that each way).  The operands of
   the small shape stay in the cache hierarchy and it sits near the launch floor; an empty-ish launch (cnt = 1 at 4x2)
   is timed beside it to show that floor.
b. the stream: FRNet.infer_stream(yuv, deinterlace) on 136x320 4:2:0 frames fed one by one (--steps input frames,
   twice as many output frames), against the same Yuv420 stream fed as many already-progressive frames as the first
   one yields; output frames per second of both, and the difference as microseconds per output frame.
c. against the parent (with --parent-root DIR, a built checkout of the parent commit): the uint8 RGB stream and the
   Yuv420 stream on this tree and on the parent's, in child processes that alternate.  "At the parent's rate" holds
   only if the two min-max ranges overlap; that is what is recorded.

    python tools/time_deinterlace.py [--repeats 7] [--parent-root DIR] [--out profiles/deinterlace.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C, H, W, SCALE, DEG = 3, 136, 320, 4, 'BD'
SUB = {'420': (2, 2), '422': (2, 1), '444': (1, 1)}


def samples(h, w, chroma):
    sx, sy = SUB[chroma]
    return h * w + 2 * ((h + sy - 1) // sy) * ((w + sx - 1) // sx)


def fps_summary(times, frames):
    fps = {m: sorted(frames[m] / t for t in ts) for m, ts in times.items()}
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
        sys.exit('time_deinterlace.py: an MI355X is required (no fallback)')
    from tecogan_pytorch_amd import main as M
    from tecogan_pytorch_amd.models import define_model
    torch.manual_seed(0)
    opt = M.default_opt()
    opt.update({'is_train': False, 'dist': False, 'device': 'cuda', 'rank': 0, 'world_size': 1})
    return define_model(opt).net_G.eval()


def stream_runner(net, dev, clip, expect, **kw):
    def go():
        n = 0
        for chunk in net.infer_stream((f for f in clip), dev, **kw):
            n += chunk.copy().shape[0]
        assert n == expect, (n, expect)
    return go


def child(root, steps, regions):
    """The untouched streams on the tree at `root`: prints one JSON line with the seconds of every region."""
    import numpy as np
    import torch
    net = make_net(root)
    import tecogan_pytorch_amd
    from tecogan_pytorch_amd.models.networks import Yuv420
    assert os.path.dirname(os.path.abspath(tecogan_pytorch_amd.__file__)).startswith(os.path.abspath(root)), 'wrong tree'
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(1234)
    spec = Yuv420(H, W)
    forms = (('rgb_u8', stream_runner(net, dev, rng.integers(0, 256, (steps, H, W, C), dtype=np.uint8), steps)),
             ('yuv420', stream_runner(net, dev, rng.integers(0, 256, (steps, spec.frame_bytes), dtype=np.uint8), steps, yuv=spec)))
    for _ in range(2):
        for _, fn in forms:
            fn()
    net.check_faults()
    times = alternate(forms, regions, torch.cuda.synchronize)
    net.check_faults()
    print('CHILD ' + json.dumps(times), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=60, help='input frames of a stream region')
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--launches', type=int, default=100)
    ap.add_argument('--parent-root', dest='parent_root', type=str, default=None)
    ap.add_argument('--child-rounds', dest='child_rounds', type=int, default=3)
    ap.add_argument('--child-regions', dest='child_regions', type=int, default=5)
    ap.add_argument('--child', type=str, default=None, help=argparse.SUPPRESS)
    ap.add_argument('--commit', type=str, default=None, help='what the result records as the commit measured')
    ap.add_argument('--out', type=str, default=os.path.join(HERE, 'profiles', 'deinterlace.json'))
    args = ap.parse_args()
    if args.child is not None:
        return child(args.child, args.steps, args.child_regions)
    if args.repeats < 5:
        ap.error('--repeats must be at least 5')
    import numpy as np
    net = make_net(HERE)
    import torch
    from tecogan_pytorch_amd import _lib as L
    from tecogan_pytorch_amd.models.networks import Deinterlace, Yuv420
    from tecogan_pytorch_amd.models.networks.tecogan_nets import STREAM_SLOTS, stream_batch_sizes
    dev = torch.device('cuda', 0)
    sync = torch.cuda.synchronize
    lib, st = L.lib(), torch.cuda.current_stream().cuda_stream
    result = {'protocol': 'kernel: back-to-back launches between two device events (launch overhead included); streams: '
                          'host frames in one by one, every chunk copied out of its ring slot, host clock around regions that '
                          'end in a synchronisation; profiler off; the forms alternate in one process',
              'commit': args.commit, 'lr_size': f'{C}x{H}x{W}', 'scale': SCALE, 'degradation': DEG, 'precision': 'fp32',
              'device': torch.cuda.get_device_name(0), 'stream_slots': STREAM_SLOTS,
              'batch_sizes_first_later': list(stream_batch_sizes())}

    def timed(fn):
        for _ in range(10):
            fn()
        sync()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.launches):
            fn()
        e1.record()
        sync()
        return e0.elapsed_time(e1) * 1e3 / args.launches            # microseconds per launch

    def summary(v):
        return {'median': statistics.median(v), 'min': min(v), 'max': max(v)}

    # -- a. the kernel ---------------------------------------------------------------------------------------------------
    K, CNT = 8, 16
    shapes = {'576x720_420_8bit': (576, 720, '420', 8), '1080x1920_422_10bit': (1080, 1920, '422', 10),
              'launch_floor_4x2_420_8bit_cnt1': (4, 2, '420', 8)}
    forms, meta, keep = {}, {}, []
    for name, (h, w, chroma, depth) in shapes.items():
        fb = samples(h, w, chroma) * (2 if depth > 8 else 1)
        cnt = 1 if name.startswith('launch_floor') else CNT
        top = (1 << depth) - 1
        src = torch.randint(0, top + 1, ((K + 1) * fb // (2 if depth > 8 else 1),), dtype=torch.int32, device=dev)
        src = src.to(torch.uint8) if depth == 8 else src.to(torch.int16).view(torch.uint8)
        dst = torch.empty(cnt * fb, dtype=torch.uint8, device=dev)
        moved = cnt * 3 * fb                                         # about two frames read and one written per output
        a, b = torch.empty(moved // 2, dtype=torch.uint8, device=dev), torch.empty(moved // 2, dtype=torch.uint8, device=dev)
        keep += [src, dst, a, b]
        fn = lambda src=src, dst=dst, h=h, w=w, c=L.YUV_CHROMA[chroma], d=depth, cnt=cnt: lib.tg_deinterlace_planar(
            src.data_ptr(), dst.data_ptr(), K, h, w, c, d, 1, 1, 0, 1, cnt, st)
        assert fn() == L.TG_OK, name
        forms[name], forms['copy_' + name] = fn, (lambda a=a, b=b: b.copy_(a))
        meta[name] = {'frames_in': K + 1, 'frames_out': cnt, 'frame_bytes': fb, 'bytes_read_plus_written': moved,
                      'copy_bytes_each_way': moved // 2}
    us = {name: [] for name in forms}
    for _ in range(args.repeats):
        for name, fn in forms.items():
            us[name].append(timed(fn))
    for name, m in meta.items():
        m['us_per_launch'], m['copy_us_per_launch'] = summary(us[name]), summary(us['copy_' + name])
        m['us_per_launch_all'], m['copy_us_per_launch_all'] = us[name], us['copy_' + name]
        m['ratio_over_copy'] = m['us_per_launch']['median'] / m['copy_us_per_launch']['median']
        m['gb_per_s'] = m['bytes_read_plus_written'] / m['us_per_launch']['median'] / 1e3
    result['kernel'] = {'launches_per_region': args.launches, 'forms': meta}
    print(json.dumps({k: (round(v['us_per_launch']['median'], 2), round(v['copy_us_per_launch']['median'], 2),
                          round(v['gb_per_s'], 1)) for k, v in meta.items()}), flush=True)
    del forms, keep

    # -- b. the stream ---------------------------------------------------------------------------------------------------
    rng = np.random.default_rng(1234)
    spec = Yuv420(H, W)
    inter = rng.integers(0, 256, (args.steps, spec.frame_bytes), dtype=np.uint8)
    prog = rng.integers(0, 256, (2 * args.steps, spec.frame_bytes), dtype=np.uint8)
    sforms = (('yuv420_deinterlace_field', stream_runner(net, dev, inter, 2 * args.steps, yuv=spec, deinterlace=Deinterlace())),
              ('yuv420_progressive', stream_runner(net, dev, prog, 2 * args.steps, yuv=spec)))
    for _ in range(2):
        for _, fn in sforms:
            fn()
    net.check_faults()
    times = alternate(sforms, args.repeats, sync)
    net.check_faults()
    result['stream'] = fps_summary(times, {name: 2 * args.steps for name, _ in sforms})
    result['stream']['unit'] = 'output frames per second'
    med = {m: statistics.median(ts) for m, ts in times.items()}
    result['stream']['cost_us_per_output_frame'] = (med['yuv420_deinterlace_field'] - med['yuv420_progressive']) / (2 * args.steps) * 1e6
    result['stream']['ranges_overlap'] = bool(
        result['stream']['fps_min']['yuv420_deinterlace_field'] <= result['stream']['fps_max']['yuv420_progressive'] and
        result['stream']['fps_min']['yuv420_progressive'] <= result['stream']['fps_max']['yuv420_deinterlace_field'])
    print(json.dumps({k: result['stream'][k] for k in ('fps_median', 'fps_min', 'fps_max', 'cost_us_per_output_frame')}), flush=True)

    # -- c. the untouched streams, this tree against the parent's ------------------------------------------------------------
    if args.parent_root:
        roots = {'parent': os.path.abspath(args.parent_root), 'this': HERE}
        secs = {path: {k: [] for k in roots} for path in ('rgb_u8', 'yuv420')}
        del net
        torch.cuda.empty_cache()
        for _ in range(args.child_rounds):
            for k, root in roots.items():
                r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', root, '--steps', str(args.steps),
                                    '--child-regions', str(args.child_regions)], capture_output=True, text=True,
                                   timeout=300, env=dict(os.environ, PYTHONPATH=root))
                line = [ln for ln in r.stdout.splitlines() if ln.startswith('CHILD ')]
                if r.returncode != 0 or not line:
                    sys.exit('time_deinterlace.py: the %s child failed (%d): %s' % (k, r.returncode, r.stderr[-2000:]))
                for path, ts in json.loads(line[0][6:]).items():
                    secs[path][k] += ts
        result['against_parent'] = {}
        for path, by_tree in secs.items():
            un = fps_summary(by_tree, {k: args.steps for k in by_tree})
            un['min_max_ranges_overlap'] = bool(un['fps_min']['this'] <= un['fps_max']['parent'] and
                                                un['fps_min']['parent'] <= un['fps_max']['this'])
            un['ratio_this_over_parent'] = un['fps_median']['this'] / un['fps_median']['parent']
            result['against_parent'][path] = un
        result['against_parent']['protocol'] = ('%d child processes per tree, alternating parent / this, each warmed and timing %d '
                                                'alternating regions of the uint8 RGB stream and of the Yuv420 stream'
                                                % (args.child_rounds, args.child_regions))
        print(json.dumps({p: {k: u[k] for k in ('fps_median', 'fps_min', 'fps_max', 'min_max_ranges_overlap')}
                          for p, u in result['against_parent'].items() if p != 'protocol'}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
