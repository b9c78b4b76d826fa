#!/usr/bin/env python3
"""What the planar YUV layouts cost.  The protocol is tools/time_yuv_depth.py's: 3x134x320 LR, 4x BD,
fp32, every form warmed, --repeats alternating regions of each in ONE process, profiler off; kernels between two device
events, streams under the host clock around regions that end in a synchronisation; medians and min-max.  Needs a GPU:
there is no fallback.

1. kernels: every form of the three entry points alone -- layout x siting x wide / element-wide (the base one sample
   off), 8 and 10 bits -- n = 1 at 536x1280 (the output direction) and at 134x320 (the input direction), --launches
   launches back to back, against a device copy that moves the same bytes (half of read + written each way).
2. the four 4:2:0 entry points (`old_*`: their own host path over the same kernels), wide and element-wide, alternate
   with the planar ones in the same regions; reported: whether the planar median lies inside the old min-max.  With
   --parent-root the parent's library is loaded beside this one and its four entry points (`parent_old_*`) alternate in
   the same regions too; reported per form: whether this tree's median lies inside the parent's min-max.  Nothing is
   asserted.
3. stream: FRNet.infer_stream fed host frames one by one, every chunk copied: 420 -> 420 with a Yuv420 at 8 bits and
   with out_depth = 10, 420 -> 444, 422p10 -> 422p10 and 444 -> 444 with a Yuv.
4. against the parent (with --parent-root DIR, a built checkout of the parent commit): the uint8 RGB stream (the control)
   and the two Yuv420 streams on this tree and on the parent's, in child processes that alternate.  Acceptance is section
   7d's rule: the new median lies inside the parent's min-max.

    python tools/time_yuv_planar.py [--repeats 7] [--parent-root DIR] [--out profiles/yuv_planar.json]
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
SUB = {'420': (2, 2), '422': (2, 1), '444': (1, 1)}


def samples(h, w, chroma):
    sx, sy = SUB[chroma]
    return h * w + 2 * ((h + sy - 1) // sy) * ((w + sx - 1) // sx)


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
        sys.exit('time_yuv_planar.py: an MI355X is required (no fallback)')
    from tecogan_pytorch_amd import main as M
    from tecogan_pytorch_amd.models import define_model
    torch.manual_seed(0)
    opt = M.default_opt()
    opt.update({'is_train': False, 'dist': False, 'device': 'cuda', 'rank': 0, 'world_size': 1})
    return define_model(opt).net_G.eval()


def child(root, steps, regions):
    """The control and the two Yuv420 streams on the tree at `root`: prints one JSON line with the seconds of every
    region."""
    import numpy as np
    import torch
    net = make_net(root)
    import tecogan_pytorch_amd
    from tecogan_pytorch_amd.models.networks import Yuv420
    assert os.path.dirname(os.path.abspath(tecogan_pytorch_amd.__file__)).startswith(os.path.abspath(root)), 'wrong tree'
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(1234)
    rgb_clip = rng.integers(0, 256, (steps, H, W, C), dtype=np.uint8)
    spec = Yuv420(H, W)
    yuv_clip = rng.integers(0, 256, (steps, spec.frame_bytes), dtype=np.uint8)

    def run(clip, **kw):
        def go():
            n = 0
            for chunk in net.infer_stream((f for f in clip), dev, **kw):
                n += chunk.copy().shape[0]
            assert n == steps
        return go
    forms = (('rgb_u8', run(rgb_clip)), ('yuv420', run(yuv_clip, yuv=spec)),
             ('yuv420_out10', run(yuv_clip, yuv=Yuv420(H, W, out_depth=10))))
    for _ in range(2):
        for _, fn in forms:
            fn()
    net.check_faults()
    times = alternate(forms, regions, torch.cuda.synchronize)
    net.check_faults()
    print('CHILD ' + json.dumps(times), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=60)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--parent-root', dest='parent_root', type=str, default=None)
    ap.add_argument('--child-rounds', dest='child_rounds', type=int, default=3)
    ap.add_argument('--child-regions', dest='child_regions', type=int, default=5)
    ap.add_argument('--child', type=str, default=None, help=argparse.SUPPRESS)
    ap.add_argument('--out', type=str, default=os.path.join(HERE, 'profiles', 'yuv_planar.json'))
    args = ap.parse_args()
    if args.child is not None:
        return child(args.child, args.steps, args.child_regions)
    if args.repeats < 5:
        ap.error('--repeats must be at least 5')
    import numpy as np
    net = make_net(HERE)
    import torch
    from tecogan_pytorch_amd import _lib as L
    from tecogan_pytorch_amd.models.networks import Yuv, Yuv420
    from tecogan_pytorch_amd.models.networks.tecogan_nets import STREAM_SLOTS, stream_batch_sizes
    dev = torch.device('cuda', 0)
    sync = torch.cuda.synchronize
    lib, st = L.lib(), torch.cuda.current_stream().cuda_stream
    result = {'protocol': 'kernels: n = 1, back-to-back launches between two device events (launch overhead included, the '
                          'operands stay in the cache hierarchy); streams: host frames in one by one, every chunk copied out '
                          'of its ring slot, host clock around regions that end in a synchronisation; profiler off; the forms '
                          'alternate in one process',
              'lr_size': f'{C}x{H}x{W}', 'scale': SCALE, 'degradation': DEG, 'precision': 'fp32',
              'device': torch.cuda.get_device_name(0), 'stream_slots': STREAM_SLOTS,
              'batch_sizes_first_later': list(stream_batch_sizes())}

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

    def summary(us):
        return {k: {'median': statistics.median(v), 'min': min(v), 'max': max(v)} for k, v in us.items()}

    # -- 1. and 2. the kernels -----------------------------------------------------------------------------------------------
    HH, WW = SCALE * H, SCALE * W
    big = 4 * 3 * HH * WW + 64
    rgb_f = torch.rand(big // 4, device=dev)                         # fp32 RGB, 16 floats of slack for the offset forms
    rgb_8 = torch.randint(0, 256, (3 * HH * WW + 64,), dtype=torch.uint8, device=dev)
    yuv_b = torch.randint(0, 256, (2 * 3 * HH * WW + 64,), dtype=torch.uint8, device=dev)      # any layout, either depth
    K = {'420': L.TG_YUV_420, '422': L.TG_YUV_422, '444': L.TG_YUV_444}
    forms, meta = {}, {}

    def add(name, fn, read_b, write_b):
        assert fn() == L.TG_OK, name
        forms[name], meta[name] = fn, {'bytes_read': read_b, 'bytes_written': write_b}

    for chroma in ('420', '422', '444'):
        for siting, sc in (('center', 0), ('left', 1)):
            if chroma == '444' and siting == 'left':
                continue                                            # (one form: the siting is not looked at)
            for wide in (True, False):
                tag = f'{chroma}_{siting}_{"wide" if wide else "elem"}'
                o1, o2 = (0, 0) if wide else (1, 2)                  # the samples' base one sample off the wide alignment
                ns_o, ns_i = samples(HH, WW, chroma), samples(H, W, chroma)
                add('out8_' + tag, lambda c=K[chroma], s=sc, o=o1: lib.tg_rgb_u8_to_yuv_planar(
                    rgb_8.data_ptr(), yuv_b.data_ptr() + o, 1, HH, WW, c, 1, 0, s, st), 3 * HH * WW, ns_o)
                add('out10_' + tag, lambda c=K[chroma], s=sc, o=o2: lib.tg_rgb_f32_to_yuv_planar16(
                    rgb_f.data_ptr(), yuv_b.data_ptr() + o, 1, HH, WW, c, 10, 1, 0, s, st), 12 * HH * WW, 2 * ns_o)
                add('in8_' + tag, lambda c=K[chroma], s=sc, o=o1: lib.tg_yuv_planar_to_rgb_f32(
                    yuv_b.data_ptr() + o, rgb_f.data_ptr(), 1, H, W, c, 8, 1, 0, s, st), ns_i, 12 * H * W)
                add('in10_' + tag, lambda c=K[chroma], s=sc, o=o2: lib.tg_yuv_planar_to_rgb_f32(
                    yuv_b.data_ptr() + o, rgb_f.data_ptr(), 1, H, W, c, 10, 1, 0, s, st), 2 * ns_i, 12 * H * W)
    ns_o, ns_i = samples(HH, WW, '420'), samples(H, W, '420')
    libs = {'old_': lib}
    if args.parent_root:                                             # the parent's library beside this one, same process
        import ctypes
        plib = ctypes.CDLL(os.path.join(os.path.abspath(args.parent_root), 'tecogan-pytorch_amd', 'libtecogan_hip.so'))
        for fn in ('tg_rgb_u8_to_yuv420', 'tg_rgb_f32_to_yuv420p16', 'tg_yuv420_to_rgb_f32', 'tg_yuv420p16_to_rgb_f32'):
            getattr(plib, fn).restype, getattr(plib, fn).argtypes = L.SIGNATURES[fn]
        libs['parent_old_'] = plib
    for pre, lb in libs.items():                                     # the four 4:2:0 entry points, wide and element-wide
        for siting, sc in (('center', 0), ('left', 1)):
            for wide in (True, False):
                tag = f'420_{siting}_{"wide" if wide else "elem"}'
                o1, o2 = (0, 0) if wide else (1, 2)
                add(f'{pre}out8_{tag}', lambda s=sc, o=o1, lb=lb: lb.tg_rgb_u8_to_yuv420(
                    rgb_8.data_ptr(), yuv_b.data_ptr() + o, 1, HH, WW, 1, 0, s, st), 3 * HH * WW, ns_o)
                add(f'{pre}out10_{tag}', lambda s=sc, o=o2, lb=lb: lb.tg_rgb_f32_to_yuv420p16(
                    rgb_f.data_ptr(), yuv_b.data_ptr() + o, 1, HH, WW, 10, 1, 0, s, st), 12 * HH * WW, 2 * ns_o)
                add(f'{pre}in8_{tag}', lambda s=sc, o=o1, lb=lb: lb.tg_yuv420_to_rgb_f32(
                    yuv_b.data_ptr() + o, rgb_f.data_ptr(), 1, H, W, 1, 0, s, st), ns_i, 12 * H * W)
                add(f'{pre}in10_{tag}', lambda s=sc, o=o2, lb=lb: lb.tg_yuv420p16_to_rgb_f32(
                    yuv_b.data_ptr() + o, rgb_f.data_ptr(), 1, H, W, 10, 1, 0, s, st), 2 * ns_i, 12 * H * W)
    copies = {}
    for name, m in meta.items():
        half = (m['bytes_read'] + m['bytes_written']) // 2
        if half not in copies:
            a, b = torch.empty(half, dtype=torch.uint8, device=dev), torch.empty(half, dtype=torch.uint8, device=dev)
            copies[half] = lambda a=a, b=b: b.copy_(a)
        m['copy_bytes_each_way'] = half
    us = {name: [] for name in forms}
    us_copy = {half: [] for half in copies}
    for _ in range(args.repeats):
        for name, fn in forms.items():
            us[name].append(timed(fn))
        for half, fn in copies.items():
            us_copy[half].append(timed(fn))
    ks, cs = summary(us), summary(us_copy)
    for name, m in meta.items():
        m['us_per_launch'] = ks[name]
        m['us_per_launch_all'] = us[name]
        m['copy_us_per_launch'] = cs[m['copy_bytes_each_way']]
        m['ratio_over_copy'] = ks[name]['median'] / cs[m['copy_bytes_each_way']]['median']
        m['gb_per_s'] = (m['bytes_read'] + m['bytes_written']) / ks[name]['median'] / 1e3
    result['kernels'] = {'out_size': f'{HH}x{WW}', 'in_size': f'{H}x{W}', 'launches_per_region': args.launches, 'forms': meta}
    versus = {}
    for name in meta:
        if name.startswith('old_'):
            new = name[4:]
            versus[new] = {'new_us': ks[new], 'old_us': ks[name],
                           'new_median_inside_old_min_max': bool(ks[name]['min'] <= ks[new]['median'] <= ks[name]['max']),
                           'ratio_new_over_old': ks[new]['median'] / ks[name]['median']}
    result['templates_against_existing_kernels'] = versus
    fold = {name[7:]: {'this_us': ks[name[7:]], 'parent_us': ks[name],
                       'this_median_inside_parent_min_max': bool(ks[name]['min'] <= ks[name[7:]]['median'] <= ks[name]['max']),
                       'ratio_this_over_parent': ks[name[7:]]['median'] / ks[name]['median']}
            for name in meta if name.startswith('parent_')}
    if fold:
        result['old_entry_points_against_parent'] = fold
        print(json.dumps({k: (v['this_median_inside_parent_min_max'], round(v['ratio_this_over_parent'], 3))
                          for k, v in fold.items()}), flush=True)
    print(json.dumps({k: (round(v['us_per_launch']['median'], 3), round(v['ratio_over_copy'], 3)) for k, v in meta.items()}), flush=True)
    print(json.dumps(versus), flush=True)
    del rgb_f, rgb_8, yuv_b, copies

    # -- 3. the stream -----------------------------------------------------------------------------------------------------
    rng = np.random.default_rng(1234)
    specs = {'yuv420_to_420_Yuv420': Yuv420(H, W), 'yuv420_to_420p10_Yuv420': Yuv420(H, W, out_depth=10),
             'yuv_420_to_444': Yuv(H, W, out_chroma='444'),
             'yuv_422p10_to_422p10': Yuv(H, W, chroma='422', depth=10), 'yuv_444_to_444': Yuv(H, W, chroma='444')}
    clips = {k: (rng.integers(0, 256, (args.steps, s.frame_bytes), dtype=np.uint8) if s.depth == 8 else
                 rng.integers(0, 1024, (args.steps, s.frame_bytes // 2), dtype=np.uint16).view(np.uint8))
             for k, s in specs.items()}

    def runner(name):
        def run():
            n = 0
            for chunk in net.infer_stream((f for f in clips[name]), dev, yuv=specs[name]):
                n += chunk.copy().shape[0]
            assert n == args.steps
        return run
    sforms = tuple((name, runner(name)) for name in specs)
    for _ in range(2):
        for _, fn in sforms:
            fn()
    net.check_faults()
    result['stream'] = fps_summary(alternate(sforms, args.repeats, sync), args.steps)
    net.check_faults()
    result['stream']['bytes_per_lr_frame'] = {k: s.frame_bytes for k, s in specs.items()}
    result['stream']['bytes_per_hr_frame'] = {k: s.out_frame_bytes(SCALE) for k, s in specs.items()}
    print(json.dumps({k: result['stream'][k] for k in ('fps_median', 'fps_min', 'fps_max')}), flush=True)

    # -- 4. the streams, this tree against the parent's -------------------------------------------------------------------------
    if args.parent_root:
        roots = {'parent': os.path.abspath(args.parent_root), 'this': HERE}
        secs = {path: {k: [] for k in roots} for path in ('rgb_u8', 'yuv420', 'yuv420_out10')}
        del net
        torch.cuda.empty_cache()
        for _ in range(args.child_rounds):
            for k, root in roots.items():
                r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', root, '--steps', str(args.steps),
                                    '--child-regions', str(args.child_regions)], capture_output=True, text=True,
                                   timeout=300, env=dict(os.environ, PYTHONPATH=root))
                line = [ln for ln in r.stdout.splitlines() if ln.startswith('CHILD ')]
                if r.returncode != 0 or not line:
                    sys.exit('time_yuv_planar.py: the %s child failed (%d): %s' % (k, r.returncode, r.stderr[-2000:]))
                for path, ts in json.loads(line[0][6:]).items():
                    secs[path][k] += ts
        result['against_parent'] = {}
        for path, by_tree in secs.items():
            un = fps_summary(by_tree, args.steps)
            un['this_median_inside_parent_min_max'] = bool(un['fps_min']['parent'] <= un['fps_median']['this'] <= un['fps_max']['parent'])
            un['ratio_this_over_parent'] = un['fps_median']['this'] / un['fps_median']['parent']
            result['against_parent'][path] = un
        result['against_parent']['protocol'] = ('%d child processes per tree, alternating parent / this, each warmed and timing %d '
                                           'alternating regions of the uint8 RGB stream and of the two Yuv420 streams'
                                           % (args.child_rounds, args.child_regions))
        print(json.dumps({p: {k: u[k] for k in ('fps_median', 'fps_min', 'fps_max', 'this_median_inside_parent_min_max')}
                          for p, u in result['against_parent'].items() if p != 'protocol'}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
