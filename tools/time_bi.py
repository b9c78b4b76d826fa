#!/usr/bin/env python3
"""What the BI degradation on the GPU costs: ops.downsample_bi against the only comparable code
the project had before it -- dequantize_u8_hwc + downsample_bd on the same frames -- and against a device copy that
moves the same bytes.  Two shapes, scale 4:

  test:   100 frames of 720x1280x3 uint8 -> fp32 LR (pad=True);
  train:  n * t = 4 * 10 crops of (128 + 16)^2 -> fp32 LR (pad=False), from the fp32 NCHW batch DeviceClipStore.gather
          delivers (BD: crops of (128 + 8)^2, its own border).

The BI and BD forms go through their ops.* wrappers (at the training shape the launches take microseconds and the
wrappers' host time is part of what is measured).  Every form is warmed; --repeats regions of --launches launches each,
the forms alternating in ONE process, profiler off, device events around each region; medians with min-max per launch.
The copy (tg_copy_ceiling, launched with the BI kernel's own grid) reads and writes (bytes in + bytes out) / 2 each.
Needs a GPU: there is no fallback.

    python tools/time_bi.py [--repeats 9] [--launches 20] [--out profiles/bi_degradation.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCALE, SIGMA = 4, 1.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--out', type=str, default=os.path.join(ROOT, 'profiles', 'bi_degradation.json'))
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error('--repeats must be at least 5')
    import torch
    if not torch.cuda.is_available():
        sys.exit('time_bi.py: an MI355X is required (no fallback)')
    from tecogan_pytorch_amd import _lib as L, ops
    from tecogan_pytorch_amd.utils.data_utils import gaussian_kernel2d
    dev = torch.device('cuda', 0)
    kern = gaussian_kernel2d(SIGMA)
    s = SCALE
    th, tw = ops.BI_TILE

    def region(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(args.launches):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / args.launches            # microseconds per call

    def measure(forms):
        for _, fn in forms:                                          # warm-up: code objects, allocator
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name, _ in forms}
        for _ in range(args.repeats):
            for name, fn in forms:
                times[name].append(region(fn))
        return {name: {'us_median': statistics.median(v), 'us_min': min(v), 'us_max': max(v), 'us_all': v}
                for name, v in times.items()}

    def copy_form(nbytes, blocks):
        half = (nbytes // 2 + 15) // 16 * 16
        src = torch.empty(half, dtype=torch.uint8, device=dev).random_(0, 256)
        dst = torch.empty_like(src)
        lib = L.lib()

        def run():
            L.check(lib.tg_copy_ceiling(src.data_ptr(), dst.data_ptr(), half, blocks, 256, ops._stream()), 'tg_copy_ceiling')
        return run, half

    def compare(rec, bytes_in, bytes_out):
        bi, bd, cp = rec['bi'], rec['bd_pair'], rec['copy_same_bytes']
        spread = (bi['us_max'] - bi['us_min']) + (bd['us_max'] - bd['us_min'])
        rec['bytes'] = {'in': bytes_in, 'out': bytes_out}
        rec['bi_GBps_of_compulsory_bytes'] = (bytes_in + bytes_out) / bi['us_median'] * 1e-3
        rec['bi_fraction_of_copy'] = cp['us_median'] / bi['us_median']
        rec['bd_pair_over_bi'] = bd['us_median'] / bi['us_median']
        rec['min_max_spread_of_both_us'] = spread
        rec['bi_not_slower_than_bd_pair_beyond_spread'] = bool(bi['us_median'] - bd['us_median'] <= spread)
        return rec

    g = torch.Generator(device='cpu').manual_seed(7)
    result = {'protocol': 'every form warmed; regions of %d launches between device events, the forms alternating in one '
                          'process, profiler off; microseconds per call (bd_pair: per pair of launches)' % args.launches,
              'device': torch.cuda.get_device_name(0), 'scale': s, 'tile_lr_pixels': [th, tw], 'repeats': args.repeats}

    # -- test shape ------------------------------------------------------------------------------------------------------
    n, H, W = 100, 720, 1280
    frames = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, generator=g).to(dev)
    oh, ow = H // s, W // s
    bytes_in, bytes_out = n * H * W * 3, n * oh * ow * 3 * 4
    blocks = n * -(-oh // th) * -(-ow // tw)
    run_copy, half = copy_form(bytes_in + bytes_out, blocks)
    rec = measure([('bi', lambda: ops.downsample_bi(frames, s, pad=True)),
                   ('bd_pair', lambda: ops.downsample_bd(ops.dequantize_u8_hwc(frames), kern, s, True)),
                   ('copy_same_bytes', run_copy)])
    rec.update({'shape': f'{n}x{H}x{W}x3 uint8 -> {n}x3x{oh}x{ow} fp32', 'workgroups': blocks,
                'copy_bytes_read_and_written_each': half})
    result['test_720p'] = compare(rec, bytes_in, bytes_out)
    print(json.dumps(result['test_720p']), flush=True)
    del frames

    # -- training shape ---------------------------------------------------------------------------------------------------
    nt, crop = 4 * 10, 128
    gb, gd = crop + 4 * s, crop + 2 * int(SIGMA * 3.0)
    crops_bi = (torch.randint(0, 256, (nt, 3, gb, gb), generator=g).float() / 255.0).to(dev)
    crops_bd = crops_bi[..., :gd, :gd].contiguous()
    ol = crop // s
    bytes_in, bytes_out = nt * 3 * gb * gb * 4, nt * 3 * ol * ol * 4
    blocks = nt * -(-ol // th) * -(-ol // tw)
    run_copy, half = copy_form(bytes_in + bytes_out, blocks)
    rec = measure([('bi', lambda: ops.downsample_bi(crops_bi, s, pad=False)),
                   ('bd_pair', lambda: ops.downsample_bd(crops_bd, kern, s, False)),
                   ('copy_same_bytes', run_copy)])
    rec.update({'shape': f'{nt}x3x{gb}x{gb} fp32 -> {nt}x3x{ol}x{ol} fp32 (bd: {nt}x3x{gd}x{gd}, one launch: the batch '
                         f'is fp32 already)', 'workgroups': blocks, 'copy_bytes_read_and_written_each': half})
    result['train_crop128'] = compare(rec, bytes_in, bytes_out)
    print(json.dumps(result['train_crop128']), flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
