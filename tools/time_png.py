#!/usr/bin/env python3
"""What PNG files encoded on the device cost and weigh.  The protocol is tools/time_yuv.py's: a
60-frame HOST clip at 3x134x320 (4x BD, fp32), both forms warmed, --repeats alternating regions of each in ONE
process, profiler off, host clock around regions that end in a synchronisation; medians, min-max and the ratio.
Needs a GPU: there is no fallback.

1. cli: `--mode infer` from a PNG folder to a PNG folder on a RAM-backed directory with `--png-encoder device` against
   `--png-encoder pillow` (the path that existed before; time_yuv.py's png_folder form on the same frames).  ONE model
   is shared by every region (main.define_model is replaced by a function that returns it).
2. stream: FRNet.infer_stream(png=Png()) fed uint8 RGB frames one by one, every yielded view copied, against
   FRNet.infer_stream yielding RGB frames, every chunk copied.
3. size: the mean file size over the clip's super-resolved frames, against Pillow at compress_level=1 and at its
   default -- for the timing clip (the output of random weights on uniform noise) and for a smooth synthetic clip.
   Neither is footage.
4. untouched: --baseline-only (with --root, a checkout of another commit) times infer_stream WITHOUT png alone and
   writes its record; --untouched PARENT NEW PARENT NEW takes four such records (one job, that order) and applies
   DESIGN.md section 7d's rule.  --bench takes `name=frames/s` figures of bench.py from the same job.

    python tools/time_png.py [--repeats 7] [--out profiles/png_encode.json]
"""
import argparse
import io
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

C, H, W, SCALE, DEG = 3, 134, 320, 4, 'BD'


def summary(times, frames, a, b):
    """times: {name: [seconds]} of the two forms a (new) and b (existing) -> the record of one comparison."""
    fps = {m: sorted(frames / t for t in ts) for m, ts in times.items()}
    med = {m: statistics.median(v) for m, v in fps.items()}
    return {'frames': frames, 'repeats': len(times[a]), 'fps_median': med, 'fps_min': {m: v[0] for m, v in fps.items()},
            'fps_max': {m: v[-1] for m, v in fps.items()}, 'fps_all': fps,
            'ratio_%s_over_%s' % (a, b): med[a] / med[b]}


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


def untouched_rule(records):
    """records: parent, new, parent, new (each {'fps_median', 'fps_min', 'fps_max'}).  Section 7d: a new median inside
    the min-max of the parent's repeats passes; one below it fails only if it is below by more than the two parent
    runs differ."""
    parents, news = records[0::2], records[1::2]
    lo, hi = min(p['fps_min'] for p in parents), max(p['fps_max'] for p in parents)
    differ = abs(parents[0]['fps_median'] - parents[1]['fps_median'])
    verdicts = []
    for r in news:
        m = r['fps_median']
        verdicts.append('inside' if lo <= m <= hi else 'above' if m > hi else
                        'below, within what the parents differ' if lo - m <= differ else 'FAILS')
    return {'parent': parents, 'new': news, 'parent_min_max': [lo, hi], 'parents_differ_by': differ,
            'new_medians': verdicts, 'passes': 'FAILS' not in verdicts}


def smooth_frames(np, t):
    """A synthetic smooth clip: gradients and a slowly moving wave, uint8 (t, H, W, 3)."""
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    out = []
    for i in range(t):
        r = 0.5 + 0.5 * np.sin(x / 37.0 + i * 0.11) * np.cos(y / 29.0)
        g = (x + 2.0 * i) % W / W
        b = 0.5 + 0.5 * np.sin((x + y) / 53.0 - i * 0.07)
        out.append(np.stack([r, g, b], 2))
    return (np.stack(out) * 255.0).round().clip(0, 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=60)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--root', type=str, default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help='the checkout whose package is measured')
    ap.add_argument('--baseline-only', action='store_true', help='infer_stream without png alone (any commit)')
    ap.add_argument('--untouched', nargs=4, metavar='JSON', default=None,
                    help='four --baseline-only records of one job: parent, new, parent, new')
    ap.add_argument('--bench', nargs='*', metavar='NAME=FPS', default=[], help="bench.py's figures of the same job")
    ap.add_argument('--out', type=str, default=None)
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error('--repeats must be at least 5')
    sys.path.insert(0, os.path.abspath(args.root))
    out_path = args.out or os.path.join(os.path.abspath(args.root), 'profiles', 'png_encode.json')
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit('time_png.py: an MI355X is required (no fallback)')
    from PIL import Image
    from tecogan_pytorch_amd import main as M
    from tecogan_pytorch_amd.models import define_model
    from tecogan_pytorch_amd.models.networks.tecogan_nets import STREAM_SLOTS, stream_batch_sizes
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    opt = M.default_opt()
    opt.update({'is_train': False, 'dist': False, 'device': 'cuda', 'rank': 0, 'world_size': 1})
    model = define_model(opt)
    net = model.net_G.eval()
    rng = np.random.default_rng(1234)
    rgb_clip = rng.integers(0, 256, (args.steps, H, W, C), dtype=np.uint8)
    sync = torch.cuda.synchronize

    def run_rgb(keep=None):
        n = 0
        for chunk in net.infer_stream((f for f in rgb_clip), dev):
            c = chunk.copy()
            n += c.shape[0]
            if keep is not None:
                keep.append(c)
        return n

    result = {'protocol': 'host frames in one by one, every chunk / view copied out of its ring slot; profiler off; host '
                          'clock around regions that end in a synchronisation; the two forms alternate in one process',
              'lr_size': f'{C}x{H}x{W}', 'scale': SCALE, 'degradation': DEG, 'precision': 'fp32',
              'device': torch.cuda.get_device_name(0), 'stream_slots': STREAM_SLOTS,
              'batch_sizes_first_later': list(stream_batch_sizes())}

    if args.baseline_only:
        for _ in range(2):
            assert run_rgb() == args.steps
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

    from tecogan_pytorch_amd import _lib, ops
    from tecogan_pytorch_amd.models.networks import Png
    png = Png()

    def run_png(keep=None):
        n = 0
        for chunk in net.infer_stream((f for f in rgb_clip), dev, png=png):
            for view in chunk:
                c = view.copy()
                n += 1
                if keep is not None:
                    keep.append(c)
        return n

    # -- 1. the CLI forms ------------------------------------------------------------------------------------------------
    ram = '/dev/shm' if os.path.isdir('/dev/shm') and os.access('/dev/shm', os.W_OK) else None
    work = tempfile.mkdtemp(prefix='time_png_', dir=ram)
    try:
        png_in, png_out = os.path.join(work, 'lr'), os.path.join(work, 'sr')
        os.makedirs(png_in)
        for i, fr in enumerate(rgb_clip):
            Image.fromarray(fr).save(os.path.join(png_in, '%04d.png' % i))
        M.define_model = lambda _opt: model                         # one model, one set of plans, for every region

        def cli(encoder):
            def run():
                shutil.rmtree(png_out, ignore_errors=True)
                assert M.infer(opt, png_in, png_out, None, encoder) == {'': args.steps}
            return run
        for _ in range(2):
            cli('pillow')()
            cli('device')()
        times = alternate((('pillow', cli('pillow')), ('device', cli('device'))), args.repeats, sync)
        result['cli'] = summary(times, args.steps, 'device', 'pillow')
        result['cli']['directory'] = 'RAM-backed (/dev/shm)' if ram else 'the default temporary directory (no /dev/shm)'
        result['cli']['num_pad_front'] = opt['test']['num_pad_front']
        result['cli']['writer_threads'] = M.INFER_WRITER_THREADS
        print(json.dumps(result['cli']), flush=True)
    finally:
        shutil.rmtree(work, ignore_errors=True)

    # -- 2. the stream ---------------------------------------------------------------------------------------------------
    for _ in range(2):
        assert run_rgb() == args.steps and run_png() == args.steps
    net.check_faults()
    times = alternate((('rgb_u8', run_rgb), ('png', run_png)), args.repeats, sync)
    net.check_faults()
    result['stream'] = summary(times, args.steps, 'png', 'rgb_u8')
    med = result['stream']['fps_median']
    result['stream']['ms_per_batch_of_%d_added' % stream_batch_sizes()[1]] = \
        (1.0 / med['png'] - 1.0 / med['rgb_u8']) * 1e3 * stream_batch_sizes()[1]
    print(json.dumps(result['stream']), flush=True)

    # the encoder alone: one later-batch of HR frames, events around the call (the per-kernel split is rocprofv3's)
    frames = []
    run_rgb(frames)
    hr = np.concatenate(frames, 0)
    m = stream_batch_sizes()[1]
    x = torch.from_numpy(hr[:m]).to(dev)
    lib = _lib.lib()
    cap = lib.tg_png_capacity(SCALE * H, SCALE * W)
    out = torch.empty(m, cap, dtype=torch.uint8, device=dev)
    sizes = torch.empty(m, dtype=torch.int64, device=dev)
    ws = torch.empty(lib.tg_png_workspace_bytes(m, SCALE * H, SCALE * W), dtype=torch.uint8, device=dev)
    ms = []
    for i in range(3 + args.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.check(lib.tg_png_encode_u8(x.data_ptr(), m, SCALE * H, SCALE * W, png.code(), out.data_ptr(), cap,
                                        sizes.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream), 'png')
        e1.record()
        e1.synchronize()
        if i >= 3:
            ms.append(e0.elapsed_time(e1))
    result['encode_alone'] = {'frames': m, 'ms_median': statistics.median(ms), 'ms_min': min(ms), 'ms_max': max(ms),
                              'note': 'tg_png_encode_u8 on an idle device, events around the four launches'}
    print(json.dumps(result['encode_alone']), flush=True)

    # -- 3. file sizes ---------------------------------------------------------------------------------------------------
    from concurrent.futures import ThreadPoolExecutor

    def pillow_size(frame, **kw):
        buf = io.BytesIO()
        Image.fromarray(frame).save(buf, 'PNG', **kw)
        return buf.tell()

    def sizes_of(hr_frames):
        dev_sizes = []
        for i in range(0, len(hr_frames), m):
            dev_sizes += [len(b) for b in ops.png_encode(torch.from_numpy(hr_frames[i:i + m]).to(dev))]
        with ThreadPoolExecutor(max_workers=8) as pool:
            l1 = list(pool.map(lambda f: pillow_size(f, compress_level=1), hr_frames))
            dflt = list(pool.map(pillow_size, hr_frames))
        raw = hr_frames[0].size
        return {'frames': len(hr_frames), 'raw_rgb_bytes': raw, 'device_mean_bytes': statistics.mean(dev_sizes),
                'pillow_level1_mean_bytes': statistics.mean(l1), 'pillow_default_mean_bytes': statistics.mean(dflt),
                'device_over_pillow_level1': statistics.mean(dev_sizes) / statistics.mean(l1),
                'device_over_pillow_default': statistics.mean(dev_sizes) / statistics.mean(dflt)}
    result['size'] = {'note': 'synthetic clips, not footage: real video has not been measured',
                      'timing_clip_random_weights_on_noise': sizes_of(hr)}
    smooth = smooth_frames(np, 20)
    hr_smooth = np.concatenate([c.copy() for c in net.infer_stream(iter([smooth]), dev)], 0)
    result['size']['smooth_clip_random_weights'] = sizes_of(hr_smooth)
    result['size']['smooth_lr_frames_themselves_134x320'] = sizes_of(smooth)
    print(json.dumps(result['size']), flush=True)

    # -- 4. the untouched path ---------------------------------------------------------------------------------------------
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
