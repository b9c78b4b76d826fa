#!/usr/bin/env python3
"""What the raw-video front and back of the stream cost.  The protocol is tools/time_stream.py's:
a 60-frame HOST clip at 3x134x320 (4x BD, fp32), both forms warmed, --repeats alternating regions of each in ONE
process, profiler off, host clock around regions that end in a synchronisation; medians, min-max and the ratio.
Needs a GPU: there is no fallback.

1. stream: FRNet.infer_stream(yuv=Yuv420(...)) fed I420 frames one by one, against FRNet.infer_stream fed uint8 RGB
   frames one by one -- the path that existed before and that `yuv` leaves untouched.  Every chunk is copied out of its
   ring slot.  The yuv form adds two launches per batch and moves half the bytes; the expectation is a median inside
   the min-max of the RGB repeats.
2. cli: `--mode infer` from a y4m file to a y4m file against the PNG-folder form on the same frames (the y4m clip
   converted by ops.yuv420_to_rgb and rounded to uint8), both on a RAM-backed directory.  main.infer and
   main.infer_y4m_cli are called in this process with ONE model shared by every region (main.define_model is
   replaced by a function that returns it), so no region pays for building plans.

    python tools/time_yuv.py [--repeats 7] [--out profiles/yuv_stream.json]
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

C, H, W, SCALE, DEG = 3, 134, 320, 4, 'BD'


def summary(times, frames, a, b):
    """times: {name: [seconds]} of the two forms a (new) and b (existing) -> the record of one comparison."""
    fps = {m: sorted(frames / t for t in ts) for m, ts in times.items()}
    med = {m: statistics.median(v) for m, v in fps.items()}
    spread = fps[b][-1] - fps[b][0]
    return {'frames': frames, 'repeats': len(times[a]), 'fps_median': med, 'fps_min': {m: v[0] for m, v in fps.items()},
            'fps_max': {m: v[-1] for m, v in fps.items()}, 'fps_all': fps, b + '_spread_fps': spread,
            'ratio_%s_over_%s' % (a, b): med[a] / med[b],
            '%s_median_inside_%s_min_max' % (a, b): bool(fps[b][0] <= med[a] <= fps[b][-1]),
            '%s_median_below_%s_median_by_more_than_its_spread' % (a, b): bool(med[b] - med[a] > spread)}


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=60)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--out', type=str, default=os.path.join(ROOT, 'profiles', 'yuv_stream.json'))
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error('--repeats must be at least 5')
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit('time_yuv.py: an MI355X is required (no fallback)')
    from PIL import Image
    from tecogan_pytorch_amd import main as M, ops
    from tecogan_pytorch_amd.models import define_model
    from tecogan_pytorch_amd.models.networks import Yuv420
    from tecogan_pytorch_amd.models.networks.tecogan_nets import STREAM_SLOTS, stream_batch_sizes
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    opt = M.default_opt()
    opt.update({'is_train': False, 'dist': False, 'device': 'cuda', 'rank': 0, 'world_size': 1})
    model = define_model(opt)
    net = model.net_G.eval()
    spec = Yuv420(H, W)                                             # bt709, limited range, left siting
    rng = np.random.default_rng(1234)
    yuv_clip = rng.integers(0, 256, (args.steps, spec.frame_bytes), dtype=np.uint8)
    rgb_clip = rng.integers(0, 256, (args.steps, H, W, C), dtype=np.uint8)
    sync = torch.cuda.synchronize

    def run_yuv():
        n = 0
        for chunk in net.infer_stream((f for f in yuv_clip), dev, yuv=spec):
            n += chunk.copy().shape[0]
        return n

    def run_rgb():
        n = 0
        for chunk in net.infer_stream((f for f in rgb_clip), dev):
            n += chunk.copy().shape[0]
        return n

    result = {'protocol': 'host frames in one by one, every chunk copied out of its ring slot; profiler off; host clock '
                          'around regions that end in a synchronisation; the two forms alternate in one process',
              'lr_size': f'{C}x{H}x{W}', 'scale': SCALE, 'degradation': DEG, 'precision': 'fp32',
              'device': torch.cuda.get_device_name(0), 'stream_slots': STREAM_SLOTS,
              'batch_sizes_first_later': list(stream_batch_sizes()), 'yuv': repr(spec),
              'bytes_per_lr_frame': {'yuv': spec.frame_bytes, 'rgb_u8': H * W * C},
              'bytes_per_hr_frame': {'yuv': spec.out_frame_bytes(SCALE), 'rgb_u8': SCALE * H * SCALE * W * C}}

    # -- 1. the stream ---------------------------------------------------------------------------------------------------
    for _ in range(2):
        assert run_rgb() == args.steps and run_yuv() == args.steps
    net.check_faults()
    times = alternate((('rgb_u8', run_rgb), ('yuv', run_yuv)), args.repeats, sync)
    net.check_faults()
    result['stream'] = summary(times, args.steps, 'yuv', 'rgb_u8')
    print(json.dumps(result['stream']), flush=True)

    # -- 2. the CLI forms ------------------------------------------------------------------------------------------------
    ram = '/dev/shm' if os.path.isdir('/dev/shm') and os.access('/dev/shm', os.W_OK) else None
    work = tempfile.mkdtemp(prefix='time_yuv_', dir=ram)
    try:
        y4m_in, y4m_out = os.path.join(work, 'in.y4m'), os.path.join(work, 'out.y4m')
        png_in, png_out = os.path.join(work, 'lr'), os.path.join(work, 'sr')
        with open(y4m_in, 'wb') as f:
            f.write(b'YUV4MPEG2 W%d H%d F25:1 Ip A1:1 C420mpeg2\n' % (W, H))
            for fr in yuv_clip:
                f.write(b'FRAME\n' + fr.tobytes())
        lr = ops.yuv420_to_rgb(torch.from_numpy(yuv_clip).to(dev), H, W)
        lr_u8 = (lr * 255.0).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).cpu().numpy()
        os.makedirs(png_in)
        for i, fr in enumerate(lr_u8):
            Image.fromarray(fr).save(os.path.join(png_in, '%04d.png' % i))
        M.define_model = lambda _opt: model                         # one model, one set of plans, for every region

        def run_png():
            shutil.rmtree(png_out, ignore_errors=True)
            assert M.infer(opt, png_in, png_out) == {'': args.steps}

        def run_y4m():
            assert M.infer_y4m_cli(opt, y4m_in, y4m_out, 'bt709', None) == args.steps
        for _ in range(2):
            run_png()
            run_y4m()
        times = alternate((('png_folder', run_png), ('y4m', run_y4m)), args.repeats, sync)
        result['cli'] = summary(times, args.steps, 'y4m', 'png_folder')
        result['cli']['directory'] = 'RAM-backed (/dev/shm)' if ram else 'the default temporary directory (no /dev/shm)'
        result['cli']['num_pad_front'] = opt['test']['num_pad_front']
        print(json.dumps(result['cli']), flush=True)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
