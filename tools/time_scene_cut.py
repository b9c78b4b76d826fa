#!/usr/bin/env python3
"""What FRNet.infer_stream(scene_cut=SceneCut()) costs.  The profiler is off; every time is a host
clock around a region that ends in a synchronisation.  Needs a GPU: there is no fallback.

A --frames (600) frame HOST stream of ONE smooth scene at 3x134x320 (4x BD, fp32), fed frame by frame, every chunk copied
out of its ring slot: no cut is found, so every conditional fill leaves at once -- the cost every user of the option
pays on every frame.  Both forms are warmed, then --repeats (at least 7) regions of scene_cut=None and of
scene_cut=SceneCut() alternate in ONE process; medians and min-max of each are recorded.  A second pair of regions
forces a cut every 50 frames (detector off / on): what the fills that do run add.

--baseline-only measures the scene_cut=None regions alone and works on any commit that has infer_stream: the rate of
the untouched path is compared between two checkouts by running this file against each (--root), alternately, in one
job; the rule is DESIGN.md section 7d's (inside the other's min-max, or below it by no more than its two runs differ).

    python tools/time_scene_cut.py [--frames 600] [--repeats 7] [--out profiles/scene_cut.json]
    python tools/time_scene_cut.py --baseline-only --root <checkout> --out <json>

Per-kernel times come from a separate run under `rocprofv3 --kernel-trace --stats` (--frames 120 --repeats 7 is enough).
"""
import argparse
import json
import os
import statistics
import sys
import time

C, H, W, SCALE, DEG = 3, 134, 320, 4, 'BD'


def smooth_scene(torch, frames):
    """One scene: a low-frequency picture that drifts one pixel a frame, plus a little fixed texture."""
    g = torch.Generator(device='cpu').manual_seed(1234)
    coarse = torch.rand(1, C, H // 8 + 2, W // 8 + 2, generator=g)
    base = torch.nn.functional.interpolate(coarse, size=(H, W), mode='bicubic', align_corners=False)[0]
    base = (base + 0.02 * torch.rand(C, H, W, generator=g)).clamp_(0, 1)
    return torch.stack([torch.roll(base, shifts=i, dims=2) for i in range(frames)]).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=600)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--baseline-only', action='store_true')
    ap.add_argument('--root', type=str, default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument('--out', type=str, default=None)
    args = ap.parse_args()
    if args.repeats < 7:
        ap.error('--repeats must be at least 7')
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    out_path = args.out or os.path.join(root, 'profiles', 'scene_cut.json')
    import torch
    if not torch.cuda.is_available():
        sys.exit('time_scene_cut.py: an MI355X is required (no fallback)')
    from tecogan_pytorch_amd.models.networks import FRNet
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    net = FRNet(C, C, 64, 10, DEG, SCALE).to(dev).eval()
    clip = smooth_scene(torch, args.frames)

    def run(**kw):
        n = 0
        for chunk in net.infer_stream((f for f in clip), dev, **kw):
            n += chunk.copy().shape[0]
        torch.cuda.synchronize()
        assert n == args.frames
        return n

    def region(**kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(**kw)
        dt = time.perf_counter() - t0
        net.check_faults()
        return args.frames / dt

    def summary(v):
        v = sorted(v)
        return {'fps_median': statistics.median(v), 'fps_min': v[0], 'fps_max': v[-1], 'fps_all': v}

    result = {'protocol': 'host frames in, uint8 frames on the host out; profiler off; host clock around regions that end '
                          'in a synchronisation; the forms alternate in one process',
              'lr_size': f'{C}x{H}x{W}', 'scale': SCALE, 'degradation': DEG, 'precision': 'fp32',
              'device': torch.cuda.get_device_name(0), 'frames': args.frames, 'repeats': args.repeats,
              'baseline_only': bool(args.baseline_only)}

    if args.baseline_only:
        for _ in range(2):
            run()
        result['none'] = summary([region() for _ in range(args.repeats)])
    else:
        from tecogan_pytorch_amd.models.networks import SceneCut
        every50 = list(range(50, args.frames, 50))
        forms = {'none': lambda: {}, 'scene_cut': lambda: {'scene_cut': SceneCut()}}
        for _ in range(2):
            for make in forms.values():
                run(**make())
        fps = {name: [] for name in forms}
        for _ in range(args.repeats):
            for name, make in forms.items():
                kw = make()
                fps[name].append(region(**kw))
                if kw:
                    assert kw['scene_cut'].cuts == [], kw['scene_cut'].cuts      # one scene: every fill leaves at once
        for name in forms:
            result[name] = summary(fps[name])
        med = {name: result[name]['fps_median'] for name in forms}
        result['scene_cut_over_none'] = med['scene_cut'] / med['none']
        result['cost_us_per_frame'] = 1e6 * (1.0 / med['scene_cut'] - 1.0 / med['none'])
        # a forced cut every 50 frames: detector off (the fills alone), and on
        forced = {'forced_detect_off': lambda: {'scene_cut': SceneCut(detect=False, at=every50)},
                  'forced_detect_on': lambda: {'scene_cut': SceneCut(at=every50)}}
        ffps = {name: [] for name in forced}
        for _ in range(args.repeats):
            for name, make in forced.items():
                kw = make()
                ffps[name].append(region(**kw))
                assert kw['scene_cut'].cuts == every50, kw['scene_cut'].cuts
        for name in forced:
            result[name] = summary(ffps[name])
        result['forced_cuts'] = len(every50)
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'w') as f:
        json.dump(result, f, indent=1)
    print('wrote', out_path)


if __name__ == '__main__':
    main()
