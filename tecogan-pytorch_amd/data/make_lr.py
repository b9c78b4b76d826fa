"""LR frames from a tree of GT PNG sequences, on the GPU: what scripts/generate_lr_bi.m (MATLAB: modcrop +
imresize(1 / s, 'bicubic')) and scripts/resize_bd.py (Gaussian blur + stride-s decimation) of the reference do.

  python -m tecogan_pytorch_amd.data.make_lr --gt GT_DIR --out LR_DIR --degradation BI --scale 4
  python -m tecogan_pytorch_amd.data.make_lr --gt GT_DIR --out LR_DIR --degradation BD --scale 4 --sigma 1.5

`GT_DIR/<sequence>/...` holds one sequence per sub-folder (frames found recursively, png | jpg); frames directly
inside GT_DIR are one sequence of their own.  The layout is mirrored under LR_DIR, every frame written as PNG.

BI goes through ops.downsample_bi (exact integers, bytes out; DESIGN.md section 7g -- not compared with MATLAB).
BD goes through ops.downsample_bd with the reflect-padded test-time form, then float32_to_uint8 on the device
(ops.quantize_u8_hwc).  Pillow decodes and encodes; LMDBs and the bicubic up-sampled baseline are not written."""
import argparse
import os
import sys

import numpy as np


def parse_args(argv=None):
    p = argparse.ArgumentParser(prog='python -m tecogan_pytorch_amd.data.make_lr', description=__doc__.split('\n\n')[0])
    p.add_argument('--gt', required=True, help='folder of GT sequences (one sub-folder per sequence), or of frames')
    p.add_argument('--out', required=True, help='folder the LR frames are written to, same layout')
    p.add_argument('--degradation', required=True, choices=['BI', 'BD'])
    p.add_argument('--scale', required=True, type=int, choices=[2, 4])
    p.add_argument('--sigma', type=float, default=1.5, help='BD: standard deviation of the Gaussian (default 1.5)')
    p.add_argument('--chunk', type=int, default=16, help='frames per launch')
    return p.parse_args(argv)


def degrade(frames_u8, degradation, scale, sigma=1.5):
    """(n,H,W,3) uint8 device tensor -> (n,h,w,3) uint8 device tensor."""
    import torch
    from .. import ops
    from ..utils.data_utils import gaussian_kernel2d
    if degradation == 'BI':
        return ops.downsample_bi(frames_u8, scale, pad=True, out='u8')
    lr = ops.downsample_bd(ops.dequantize_u8_hwc(frames_u8), gaussian_kernel2d(sigma), scale, pad=True)
    return torch.stack([ops.quantize_u8_hwc(f) for f in lr])


def sequences(gt_dir):
    """[(sub-folder or '', [frame paths])]: main.infer_sequences' rule."""
    from ..main import infer_sequences
    return infer_sequences(gt_dir)


def make_lr(gt_dir, out_dir, degradation, scale, sigma=1.5, chunk=16):
    """Returns {sequence: frames written}."""
    import torch
    from PIL import Image
    from .folder_dataset import read_rgb
    if degradation not in ('BI', 'BD') or scale not in (2, 4):
        raise ValueError(f'make_lr: degradation {degradation!r} (BI | BD), scale {scale!r} (2 | 4)')
    seqs = sequences(gt_dir)
    if not seqs:
        raise ValueError(f'--gt {gt_dir}: no png | jpg frames, directly or one level down')
    done = {}
    for seq, files in seqs:
        root = os.path.join(gt_dir, seq) if seq else gt_dir
        k = 0
        while k < len(files):
            group = [files[k]]
            first = read_rgb(files[k])
            imgs = [first]
            while len(group) < chunk and k + len(group) < len(files):        # frames of one size share a launch
                nxt = read_rgb(files[k + len(group)])
                if nxt.shape != first.shape:
                    break
                group.append(files[k + len(group)])
                imgs.append(nxt)
            lr = degrade(torch.from_numpy(np.stack(imgs)).cuda(), degradation, scale, sigma).cpu().numpy()
            for path, frame in zip(group, lr):
                dst = os.path.join(out_dir, seq, os.path.splitext(os.path.relpath(path, root))[0] + '.png')
                os.makedirs(os.path.dirname(dst), exist_ok=True)
                Image.fromarray(np.ascontiguousarray(frame)).save(dst)
            k += len(group)
        done[seq] = k
    return done


def main(argv=None):
    args = parse_args(argv)
    done = make_lr(args.gt, args.out, args.degradation, args.scale, args.sigma, max(1, args.chunk))
    for seq, n in done.items():
        print(f'{seq or os.path.basename(os.path.normpath(args.gt))}: {n} frames -> {os.path.join(args.out, seq)}')
    return 0


if __name__ == '__main__':
    sys.exit(main())
