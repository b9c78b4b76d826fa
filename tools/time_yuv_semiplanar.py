#!/usr/bin/env python3
"""What the semi-planar YUV forms cost.  The protocol is tools/time_yuv_planar.py's: 3x134x320 LR,
4x BD, fp32, every form warmed, --repeats alternating regions of each in ONE process, profiler off; kernels between two
device events, streams under the host clock around regions that end in a synchronisation; medians and min-max.  Needs
a GPU: there is no fallback.

1. kernels: every semi-planar form of the three entry points next to its planar twin, which moves exactly the same
   bytes -- layout x siting x wide / element-wide (the base one sample off), 8 and 10 bits -- n = 1 at 536x1280 (the
   output direction) and at 134x320 (the input direction), --launches launches back to back.  Reported per form: whether
   the semi-planar median lies inside the twin's min-max, and the ratio.  With --parent-root the parent's library is
   loaded beside this one and its three planar entry points (`parent_*`) alternate in the same regions; reported per
   planar form: whether this tree's median lies inside the parent's min-max.  Nothing is asserted.
2. stream: FRNet.infer_stream fed host frames one by one, every chunk copied: a Yuv420 stream, the planar Yuv twin,
   nv12 -> nv12 and p010 -> p010 beside planar 420p10 -> 420p10.
3. against the parent (with --parent-root DIR, a built checkout of the parent commit): the uint8 RGB stream and the two
   Yuv420 streams on this tree and on the parent's, in child processes that alternate (tools/time_yuv_planar.py's
   children).  Acceptance is section 7d's rule: the new median lies inside the parent's min-max.

    python tools/time_yuv_semiplanar.py [--repeats 7] [--parent-root DIR] [--out profiles/yuv_semiplanar.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from time_yuv_planar import C, DEG, H, SCALE, W, alternate, fps_summary, make_net, samples  # noqa: E402

PLANAR_TOOL = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'time_yuv_planar.py')


def inside(new, old):
    return {'new_us': new, 'twin_us': old, 'new_median_inside_twin_min_max': bool(old['min'] <= new['median'] <= old['max']),
            'ratio_new_over_twin': new['median'] / old['median']}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=60)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--parent-root', dest='parent_root', type=str, default=None)
    ap.add_argument('--child-rounds', dest='child_rounds', type=int, default=3)
    ap.add_argument('--child-regions', dest='child_regions', type=int, default=5)
    ap.add_argument('--out', type=str, default=os.path.join(HERE, 'profiles', 'yuv_semiplanar.json'))
    args = ap.parse_args()
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

    # -- 1. the kernels ------------------------------------------------------------------------------------------------------
    HH, WW = SCALE * H, SCALE * W
    rgb_f = torch.rand(3 * HH * WW + 16, device=dev)                # fp32 RGB
    rgb_8 = torch.randint(0, 256, (3 * HH * WW + 64,), dtype=torch.uint8, device=dev)
    yuv_b = torch.randint(0, 256, (2 * 3 * HH * WW + 64,), dtype=torch.uint8, device=dev)      # any layout, either depth
    K = {'420': L.TG_YUV_420, '422': L.TG_YUV_422, '444': L.TG_YUV_444}
    libs = {'semi_': (lib, 'semiplanar'), 'planar_': (lib, 'planar')}
    if args.parent_root:                                             # the parent's library beside this one, same process
        import ctypes
        plib = ctypes.CDLL(os.path.join(os.path.abspath(args.parent_root), 'tecogan-pytorch_amd', 'libtecogan_hip.so'))
        for fn in ('tg_rgb_u8_to_yuv_planar', 'tg_rgb_f32_to_yuv_planar16', 'tg_yuv_planar_to_rgb_f32'):
            getattr(plib, fn).restype, getattr(plib, fn).argtypes = L.SIGNATURES[fn]
        libs['parent_'] = (plib, 'planar')
    forms, meta = {}, {}

    def add(name, fn, read_b, write_b):
        assert fn() == L.TG_OK, name
        forms[name], meta[name] = fn, {'bytes_read': read_b, 'bytes_written': write_b}

    for pre, (lb, lay) in libs.items():
        f_in, f_o8 = getattr(lb, f'tg_yuv_{lay}_to_rgb_f32'), getattr(lb, f'tg_rgb_u8_to_yuv_{lay}')
        f_o16 = getattr(lb, f'tg_rgb_f32_to_yuv_{lay}16')
        for chroma in ('420', '422', '444'):
            for siting, sc in (('center', 0), ('left', 1)):
                if chroma == '444' and siting == 'left':
                    continue                                        # (one form: the siting is not looked at)
                for wide in (True, False):
                    tag = f'{chroma}_{siting}_{"wide" if wide else "elem"}'
                    o1, o2 = (0, 0) if wide else (1, 2)              # the samples' base one sample off the wide alignment
                    ns_o, ns_i = samples(HH, WW, chroma), samples(H, W, chroma)
                    add(f'{pre}out8_{tag}', lambda f=f_o8, c=K[chroma], s=sc, o=o1: f(
                        rgb_8.data_ptr(), yuv_b.data_ptr() + o, 1, HH, WW, c, 1, 0, s, st), 3 * HH * WW, ns_o)
                    add(f'{pre}out10_{tag}', lambda f=f_o16, c=K[chroma], s=sc, o=o2: f(
                        rgb_f.data_ptr(), yuv_b.data_ptr() + o, 1, HH, WW, c, 10, 1, 0, s, st), 12 * HH * WW, 2 * ns_o)
                    add(f'{pre}in8_{tag}', lambda f=f_in, c=K[chroma], s=sc, o=o1: f(
                        yuv_b.data_ptr() + o, rgb_f.data_ptr(), 1, H, W, c, 8, 1, 0, s, st), ns_i, 12 * H * W)
                    add(f'{pre}in10_{tag}', lambda f=f_in, c=K[chroma], s=sc, o=o2: f(
                        yuv_b.data_ptr() + o, rgb_f.data_ptr(), 1, H, W, c, 10, 1, 0, s, st), 2 * ns_i, 12 * H * W)
    us = {name: [] for name in forms}
    for _ in range(args.repeats):
        for name, fn in forms.items():
            us[name].append(timed(fn))
    ks = {k: {'median': statistics.median(v), 'min': min(v), 'max': max(v)} for k, v in us.items()}
    for name, m in meta.items():
        m['us_per_launch'] = ks[name]
        m['us_per_launch_all'] = us[name]
        m['gb_per_s'] = (m['bytes_read'] + m['bytes_written']) / ks[name]['median'] / 1e3
    result['kernels'] = {'out_size': f'{HH}x{WW}', 'in_size': f'{H}x{W}', 'launches_per_region': args.launches, 'forms': meta}
    twins = {name[5:]: inside(ks[name], ks['planar_' + name[5:]]) for name in meta if name.startswith('semi_')}
    result['semiplanar_against_planar_twin'] = twins
    result['semiplanar_forms_outside_twin_min_max'] = sorted(k for k, v in twins.items() if not v['new_median_inside_twin_min_max'])
    print(json.dumps({k: (v['new_median_inside_twin_min_max'], round(v['new_us']['median'], 3), round(v['ratio_new_over_twin'], 3))
                      for k, v in twins.items()}), flush=True)
    if args.parent_root:
        fold = {name[7:]: {'this_us': ks['planar_' + name[7:]], 'parent_us': ks[name],
                           'this_median_inside_parent_min_max': bool(ks[name]['min'] <= ks['planar_' + name[7:]]['median'] <= ks[name]['max']),
                           'ratio_this_over_parent': ks['planar_' + name[7:]]['median'] / ks[name]['median']}
                for name in meta if name.startswith('parent_')}
        result['planar_entry_points_against_parent'] = fold
        print(json.dumps({k: (v['this_median_inside_parent_min_max'], round(v['ratio_this_over_parent'], 3))
                          for k, v in fold.items()}), flush=True)
    del rgb_f, rgb_8, yuv_b

    # -- 2. the stream -----------------------------------------------------------------------------------------------------
    rng = np.random.default_rng(1234)
    specs = {'yuv420_to_420_Yuv420': Yuv420(H, W), 'yuv_420_to_420_planar': Yuv(H, W),
             'nv12_to_nv12': Yuv(H, W, layout='semi'),
             'yuv_420p10_to_420p10_planar': Yuv(H, W, depth=10), 'p010_to_p010': Yuv(H, W, depth=10, layout='semi')}
    clips = {k: (rng.integers(0, 256, (args.steps, s.frame_bytes), dtype=np.uint8) if s.depth == 8 else
                 (rng.integers(0, 1024, (args.steps, s.frame_bytes // 2), dtype=np.uint16)
                  << (6 if s.layout == 'semi' else 0)).view(np.uint8))
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

    # -- 3. the streams, this tree against the parent's ------------------------------------------------------------------------
    if args.parent_root:
        roots = {'parent': os.path.abspath(args.parent_root), 'this': HERE}
        secs = {path: {k: [] for k in roots} for path in ('rgb_u8', 'yuv420', 'yuv420_out10')}
        del net
        torch.cuda.empty_cache()
        for _ in range(args.child_rounds):
            for k, root in roots.items():
                r = subprocess.run([sys.executable, PLANAR_TOOL, '--child', root, '--steps', str(args.steps),
                                    '--child-regions', str(args.child_regions)], capture_output=True, text=True,
                                   timeout=300, env=dict(os.environ, PYTHONPATH=root))
                line = [ln for ln in r.stdout.splitlines() if ln.startswith('CHILD ')]
                if r.returncode != 0 or not line:
                    sys.exit('time_yuv_semiplanar.py: the %s child failed (%d): %s' % (k, r.returncode, r.stderr[-2000:]))
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
