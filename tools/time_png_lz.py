#!/usr/bin/env python3
"""What the device PNG encoder's LZ77 mode costs and saves.  The protocol is tools/time_png.py's
(section 7i): a 60-frame HOST clip at 3x134x320 (4x BD, fp32), every form warmed, --repeats alternating regions of each
in ONE process, profiler off, host clock around regions that end in a synchronisation; medians and min-max.
Needs a GPU: there is no fallback.

1. cli: `--mode infer` from a PNG folder to a PNG folder on a RAM-backed directory: `--png-encoder pillow`,
   `--png-encoder device`, and the latter with `--png-lz77`.
2. stream: FRNet.infer_stream yielding RGB frames, with png=Png(), and with png=Png(lz77=True).
3. alone: tg_png_encode_u8 against tg_png_encode_lz_u8 for one later-batch of 536x1280 frames, events around the call.
4. size: mean file sizes of `device`, `device + lz77`, Pillow at compress_level=1 and Pillow's default, for the timing
   clip (random weights on uniform noise), a smooth synthetic clip and its LR frames.  Neither is footage.  No LZ file
   may be longer than the Huffman-only one: asserted per frame.
5. untouched: --baseline-only (with --root, a checkout of another commit) times infer_stream WITHOUT png and with
   Png() alone and writes its record; --untouched PARENT NEW PARENT NEW takes four such records (one job, that order)
   and applies DESIGN.md section 7d's rule to both.

    python tools/time_png_lz.py [--repeats 7] [--out profiles/png_lz77.json]
"""
import argparse
import io
import json
import os
import shutil
import statistics
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from time_png import C, DEG, H, SCALE, W, alternate, smooth_frames, untouched_rule  # noqa: E402


def rates(times, frames):
    fps = {m: sorted(frames / t for t in ts) for m, ts in times.items()}
    return {'frames': frames, 'repeats': len(next(iter(times.values()))),
            'fps_median': {m: statistics.median(v) for m, v in fps.items()}, 'fps_min': {m: v[0] for m, v in fps.items()},
            'fps_max': {m: v[-1] for m, v in fps.items()}, 'fps_all': fps}


def one(rec, name):
    return {k: (v[name] if isinstance(v, dict) else v) for k, v in rec.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=60)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--root', type=str, default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help='the checkout whose package is measured')
    ap.add_argument('--baseline-only', action='store_true', help='infer_stream without png and with Png() alone (any commit)')
    ap.add_argument('--untouched', nargs=4, metavar='JSON', default=None,
                    help='four --baseline-only records of one job: parent, new, parent, new')
    ap.add_argument('--bench', nargs='*', metavar='NAME=FPS', default=[],
                    help="bench.py's figures, parent and new alternating (a name may repeat: the figures are kept in order)")
    ap.add_argument('--out', type=str, default=None)
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error('--repeats must be at least 5')
    sys.path.insert(0, os.path.abspath(args.root))
    out_path = args.out or os.path.join(os.path.abspath(args.root), 'profiles', 'png_lz77.json')
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit('time_png_lz.py: an MI355X is required (no fallback)')
    from PIL import Image
    from tecogan_pytorch_amd import main as M
    from tecogan_pytorch_amd.models import define_model
    from tecogan_pytorch_amd.models.networks import Png
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

    def run_png(png):
        def run():
            n = 0
            for chunk in net.infer_stream((f for f in rgb_clip), dev, png=png):
                for view in chunk:
                    view.copy()
                    n += 1
            return n
        return run

    result = {'protocol': 'host frames in one by one, every chunk / view copied out of its ring slot; profiler off; host '
                          'clock around regions that end in a synchronisation; the forms alternate in one process',
              'lr_size': f'{C}x{H}x{W}', 'scale': SCALE, 'degradation': DEG, 'precision': 'fp32',
              'device': torch.cuda.get_device_name(0), 'stream_slots': STREAM_SLOTS,
              'batch_sizes_first_later': list(stream_batch_sizes())}

    if args.baseline_only:
        forms = (('rgb_u8', run_rgb), ('png', run_png(Png())))
        for _ in range(2):
            assert all(fn() == args.steps for _, fn in forms)
        rec = rates(alternate(forms, args.repeats, sync), args.steps)
        net.check_faults()
        result['untouched'] = {name: one(rec, name) for name, _ in forms}
        print(json.dumps(result['untouched']), flush=True)
        with open(out_path, 'w') as f:
            json.dump(result, f, indent=1)
        print('wrote', out_path)
        return

    from tecogan_pytorch_amd import _lib, ops
    m = stream_batch_sizes()[1]

    # -- 1. the CLI forms ------------------------------------------------------------------------------------------------
    ram = '/dev/shm' if os.path.isdir('/dev/shm') and os.access('/dev/shm', os.W_OK) else None
    work = tempfile.mkdtemp(prefix='time_png_lz_', dir=ram)
    try:
        png_in, png_out = os.path.join(work, 'lr'), os.path.join(work, 'sr')
        os.makedirs(png_in)
        for i, fr in enumerate(rgb_clip):
            Image.fromarray(fr).save(os.path.join(png_in, '%04d.png' % i))
        M.define_model = lambda _opt: model                         # one model, one set of plans, for every region

        def cli(encoder, lz77):
            def run():
                shutil.rmtree(png_out, ignore_errors=True)
                assert M.infer(opt, png_in, png_out, None, encoder, None, lz77) == {'': args.steps}
            return run
        forms = (('pillow', cli('pillow', False)), ('device', cli('device', False)), ('device_lz77', cli('device', True)))
        for _ in range(2):
            for _, fn in forms:
                fn()
        result['cli'] = rates(alternate(forms, args.repeats, sync), args.steps)
        result['cli']['directory'] = 'RAM-backed (/dev/shm)' if ram else 'the default temporary directory (no /dev/shm)'
        print(json.dumps(result['cli']), flush=True)
    finally:
        shutil.rmtree(work, ignore_errors=True)

    # -- 2. the stream ---------------------------------------------------------------------------------------------------
    forms = (('rgb_u8', run_rgb), ('png', run_png(Png())), ('png_lz77', run_png(Png(lz77=True))))
    for _ in range(2):
        assert all(fn() == args.steps for _, fn in forms)
    net.check_faults()
    result['stream'] = rates(alternate(forms, args.repeats, sync), args.steps)
    net.check_faults()
    med = result['stream']['fps_median']
    result['stream']['ms_per_batch_of_%d_added_over_rgb' % m] = {k: (1.0 / med[k] - 1.0 / med['rgb_u8']) * 1e3 * m
                                                                for k in ('png', 'png_lz77')}
    print(json.dumps(result['stream']), flush=True)

    # -- 3. the encoders alone: one later-batch of HR frames, events around the call ----------------------------------------
    frames = []
    run_rgb(frames)
    hr = np.concatenate(frames, 0)
    smooth = smooth_frames(np, 20)
    hr_smooth = np.concatenate([c.copy() for c in net.infer_stream(iter([smooth]), dev)], 0)
    lib = _lib.lib()
    hh, ww = SCALE * H, SCALE * W
    cap = lib.tg_png_capacity(hh, ww)
    out = torch.empty(m, cap, dtype=torch.uint8, device=dev)
    sizes = torch.empty(m, dtype=torch.int64, device=dev)
    ws = torch.empty(lib.tg_png_lz_workspace_bytes(m, hh, ww), dtype=torch.uint8, device=dev)
    result['encode_alone'] = {'frames': m, 'size': f'{hh}x{ww}', 'note': 'an idle device, events around the launches of one call',
                              'workspace_bytes': {'huffman_only': lib.tg_png_workspace_bytes(m, hh, ww),
                                                  'lz77': lib.tg_png_lz_workspace_bytes(m, hh, ww)}}
    for clip_name, clip in (('timing_clip', hr), ('smooth_clip', hr_smooth)):
        x = torch.from_numpy(clip[:m]).to(dev)
        ms = {'huffman_only': [], 'lz77': []}
        for i in range(3 + args.repeats):
            for name, fn in (('huffman_only', lib.tg_png_encode_u8), ('lz77', lib.tg_png_encode_lz_u8)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                _lib.check(fn(x.data_ptr(), m, hh, ww, 1, out.data_ptr(), cap, sizes.data_ptr(), ws.data_ptr(),
                              torch.cuda.current_stream().cuda_stream), name)
                e1.record()
                e1.synchronize()
                if i >= 3:
                    ms[name].append(e0.elapsed_time(e1))
        result['encode_alone'][clip_name] = {k: {'ms_median': statistics.median(v), 'ms_min': min(v), 'ms_max': max(v)}
                                             for k, v in ms.items()}
    print(json.dumps(result['encode_alone']), flush=True)

    # -- 4. file sizes ---------------------------------------------------------------------------------------------------
    from concurrent.futures import ThreadPoolExecutor

    def pillow_size(frame, **kw):
        buf = io.BytesIO()
        Image.fromarray(frame).save(buf, 'PNG', **kw)
        return buf.tell()

    def sizes_of(hr_frames):
        plain, lz = [], []
        for i in range(0, len(hr_frames), m):
            x = torch.from_numpy(hr_frames[i:i + m]).to(dev)
            plain += [len(b) for b in ops.png_encode(x)]
            files = ops.png_encode(x, lz77=True)
            lz += [len(b) for b in files]
            for k, b in enumerate(files):
                with Image.open(io.BytesIO(b)) as im:
                    assert np.array_equal(np.asarray(im), hr_frames[i + k]), 'an LZ file does not decode to its frame'
        assert all(a <= b for a, b in zip(lz, plain)), 'an LZ file is longer than the Huffman-only one'
        with ThreadPoolExecutor(max_workers=8) as pool:
            l1 = list(pool.map(lambda f: pillow_size(f, compress_level=1), hr_frames))
            dflt = list(pool.map(pillow_size, hr_frames))
        mean = statistics.mean
        return {'frames': len(hr_frames), 'raw_rgb_bytes': hr_frames[0].size, 'device_mean_bytes': mean(plain),
                'device_lz77_mean_bytes': mean(lz), 'pillow_level1_mean_bytes': mean(l1),
                'pillow_default_mean_bytes': mean(dflt), 'lz77_never_longer_per_frame': True,
                'device_lz77_over_device': mean(lz) / mean(plain), 'device_lz77_over_pillow_level1': mean(lz) / mean(l1),
                'device_lz77_over_pillow_default': mean(lz) / mean(dflt), 'device_over_pillow_level1': mean(plain) / mean(l1)}
    result['size'] = {'note': 'synthetic clips, not footage: real video has not been measured',
                      'timing_clip_random_weights_on_noise': sizes_of(hr),
                      'smooth_clip_random_weights': sizes_of(hr_smooth),
                      'smooth_lr_frames_themselves_134x320': sizes_of(smooth)}
    print(json.dumps(result['size']), flush=True)

    # -- 5. the untouched paths --------------------------------------------------------------------------------------------
    if args.untouched:
        recs = []
        for p in args.untouched:
            with open(p) as f:
                recs.append(json.load(f)['untouched'])
        result['untouched'] = {name: untouched_rule([r[name] for r in recs]) for name in ('rgb_u8', 'png')}
        print(json.dumps({name: {k: v for k, v in r.items() if k not in ('parent', 'new')}
                          for name, r in result['untouched'].items()}), flush=True)
    if args.bench:
        result['bench_py_frames_per_s'] = {}
        for name, v in (b.split('=') for b in args.bench):
            result['bench_py_frames_per_s'].setdefault(name, []).append(float(v))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'w') as f:
        json.dump(result, f, indent=1)
    print('wrote', out_path)


if __name__ == '__main__':
    main()
