"""Driver with the reference's three modes and CLI flags (codes/main.py,
codes/utils/base_utils.py:14-30): train | test | profile -- and infer, which the reference has not.

`train` reads the reference's LMDB training sets when `dataset.train.seq_dir` names one
(tecogan_pytorch_amd/data: the decoded frames live in HBM, batches are cut out by a HIP
kernel with the reference's augmentation).  `test` reads the reference's PNG folders when the
yml's `dataset.test*` entries name an existing `gt_seq_dir` (and `lr_seq_dir`, or the BD degradation of the GT, or
with `degradation.on_device` the BI one, on the device) and evaluates with the yml's `metric` section (PSNR, LPIPS).  Otherwise clips come from
a synthetic source that honours the loader's output contract (unpaired_lmdb_dataset.py:89-93,
paired_folder_dataset.py:57-63); any iterable of such dicts can be passed to `train()` / `test()`.

`infer` upscales a folder of LR frames (`--input`: the frames themselves, or one sub-folder per sequence) into
`--output` without ground truth: frames are decoded lazily, streamed through VSRModel.infer_stream in bounded memory
(any length) and written as PNGs under the input's names.  PNG decoding and encoding bound its rate: what it prints
is a codec number, not a GPU number.  `--png-encoder device` has the GPU write the PNG files
(Huffman-only deflate: larger files) and leaves the host the decoding of the input and the writes.  With an `--input` that is a y4m file or `-` (stdin) the clip is raw 8-bit YUV 4:2:0
video instead (data/y4m.py): I420 frames go up as they are, are converted on the device both ways (DESIGN.md section
7e) and leave as a y4m stream to `--output` (a file, or `-` for stdout), so a codec can sit on either side of a pipe:

  ffmpeg -i in.mp4 -f yuv4mpegpipe - | python -m tecogan_pytorch_amd.main --mode infer --input - --output - | ffmpeg -i - out.mp4

A `C420p10` / `C420p12` y4m input is taken as well (`--yuv-siting` names the chroma siting those
headers do not carry), and `--output-depth 8|10|12` (default: the input's) sets the bits per sample of the y4m written:
above 8 the frames are converted from the float result, not from the rounded 8-bit one.  `C422*` and `C444*` inputs are
taken too, `--output-chroma 420|422|444` (default: the input's) sets the layout written -- 444 keeps every chroma sample
the network computed -- and `--yuv-matrix bt2020` is the non-constant-luminance BT.2020 matrix.

`--deinterlace auto|tff|bff` (y4m input) takes `It` / `Ib` streams and deinterlaces them on the
GPU in front of the generator, at field rate (the header's `F` doubled) or with `--deinterlace-rate frame` at the
input's; without it an interlaced header is refused.  The header written says `Ip`.

`--raw-format nv12|nv16|nv24|p010|p012|p210|p212|p410|p412 --raw-size WxH [--raw-rate N:D]` takes
the input (a file, or `-`) as headerless semi-planar raw video, what hardware decoders hand over and
`ffmpeg -f rawvideo -pix_fmt nv12` writes; `--output-format raw|y4m` (default: raw for raw input, y4m for y4m input) says
what is written -- raw is semi-planar at `--output-chroma` / `--output-depth`, its format name and size named on stderr:

  ffmpeg -i in.mp4 -f rawvideo -pix_fmt nv12 - | python -m tecogan_pytorch_amd.main --mode infer --input - --raw-format nv12 --raw-size 320x134 --output - | ffmpeg -f rawvideo -pix_fmt nv12 -s 1280x536 -i - out.mp4

`--scene-cut` (both forms of `infer`) restarts the recurrence at scene cuts, detected on the
device; the cut frames are listed on stderr at the end, never on stdout.

  python -m tecogan_pytorch_amd.main --mode profile --lr_size 3x134x320 --test_speed
  python -m tecogan_pytorch_amd.main --mode infer --opt my_test.yml --input lr_frames/ --output sr_frames/
  python -m tecogan_pytorch_amd.main --mode train --opt my_train.yml --gpu_ids 0
  torchrun --nproc-per-node 8 -m tecogan_pytorch_amd.main --mode train ...   (DDP over RCCL)
"""
import argparse
import os
import random
import re
import time

import numpy as np
import torch
import yaml

from .metrics.psnr import compute_psnr, compute_psnr_device  # noqa: F401
from .models import define_model
from .models.networks import define_generator
from .utils import dist_utils


def output_size_arg(text):
    """`WxH` of --output-size -> (w, h)."""
    m = re.fullmatch(r'([1-9][0-9]*)[xX]([1-9][0-9]*)', text.strip())
    if not m:
        raise argparse.ArgumentTypeError(f'{text!r}: the output size is WxH, two positive integers')
    return int(m.group(1)), int(m.group(2))


def raw_rate_arg(text):
    """`N:D` of --raw-rate -> (n, d)."""
    m = re.fullmatch(r'([1-9][0-9]*):([1-9][0-9]*)', text.strip())
    if not m:
        raise argparse.ArgumentTypeError(f'{text!r}: the frame rate is N:D, two positive integers')
    return int(m.group(1)), int(m.group(2))


def raw_format_arg(text):
    """A --raw-format name -> its table key (`p010le` is `p010`)."""
    from .data.rawvideo import FORMAT_OF, RawVideoError, format_of
    try:
        return FORMAT_OF[format_of(text)]
    except RawVideoError as e:
        raise argparse.ArgumentTypeError(str(e)) from None


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--exp_dir', type=str, default='.')
    p.add_argument('--mode', type=str, required=True, help='train|test|profile|infer')
    p.add_argument('--opt', type=str, default=None, help='yaml config (reference schema)')
    p.add_argument('--gpu_ids', type=str, default='0')
    p.add_argument('--lr_size', type=str, default='3x256x256')
    p.add_argument('--test_speed', action='store_true')
    p.add_argument('--local_rank', default=-1, type=int)
    p.add_argument('--iters', type=int, default=None,
                   help='train iterations to run.  Default: with an LMDB training set, up to '
                        'train.total_iter of the yml (the reference\'s loop, main.py:60-66); with the '
                        'synthetic source 20')
    p.add_argument('--resume', type=int, default=0,
                   help='iteration to resume from: loads {G,D}_iter<k>.pth and state_iter<k>.pth from '
                        'train.ckpt_dir and continues at k + 1 (the reference leaves this as a TODO, '
                        'base_model.py:220-222)')
    p.add_argument('--precision', type=str, default=None, choices=['fp32', 'fp16'],
                   help="inference precision of the generator's SRNet body (overrides model.generator.precision of "
                        "the yml; absent = 'fp32').  Training is always fp32")
    p.add_argument('--input', type=str, default=None,
                   help='--mode infer: folder of LR frames (png | jpg), either the frames of one sequence or one '
                        'sub-folder per sequence; no ground truth is needed.  Or a y4m file (4:2:0 at 8, 10 or 12 bits), or - for '
                        'a y4m stream on stdin')
    p.add_argument('--output', type=str, default=None,
                   help='--mode infer: folder the super-resolved PNGs are written to, under the names (and sub-folders) '
                        'of the input.  With y4m input: the y4m file to write, or - for stdout (logging then goes to '
                        'stderr)')
    p.add_argument('--yuv-matrix', dest='yuv_matrix', type=str, default='bt709', choices=['bt601', 'bt709', 'bt2020'],
                   help='y4m input: the YCbCr matrix of the clip (y4m headers do not carry it); bt2020 is the '
                        'non-constant-luminance one (DESIGN.md section 7l)')
    p.add_argument('--yuv-range', dest='yuv_range', type=str, default=None, choices=['limited', 'full'],
                   help="y4m input: the range of the clip; default: the header's XCOLORRANGE, or limited without one")
    p.add_argument('--yuv-siting', dest='yuv_siting', type=str, default='left', choices=['center', 'left'],
                   help='y4m input: where a chroma sample sits, consulted only where the header does not decide '
                        '(C420p10, C420p12 and every C422 / C444 tag carry no siting); 8-bit 4:2:0 headers decide for '
                        'themselves')
    p.add_argument('--output-depth', dest='output_depth', type=int, default=None, choices=[8, 10, 12],
                   help="y4m input: bits per sample of the y4m written (DESIGN.md section 7k); default: the input's.  "
                        'Above 8 the frames are converted from the float result, not from the rounded 8-bit one')
    p.add_argument('--output-chroma', dest='output_chroma', type=str, default=None, choices=['420', '422', '444'],
                   help="y4m input: chroma layout of the y4m written (DESIGN.md section 7l); default: the input's.  444 "
                        'keeps every chroma sample the network computed')
    p.add_argument('--scene-cut', dest='scene_cut', action='store_true',
                   help='--mode infer: restart the recurrence at scene cuts, detected on the GPU (DESIGN.md section 7h); '
                        'the cut frames are listed on stderr at the end.  The default thresholds have not been '
                        'validated on real footage')
    p.add_argument('--scene-cut-mad', dest='scene_cut_mad', type=float, default=24.0,
                   help='--scene-cut: least mean absolute luma difference of a cut, in 8-bit levels')
    p.add_argument('--scene-cut-hist', dest='scene_cut_hist', type=float, default=0.25,
                   help='--scene-cut: least distance of the two 32-bin luma histograms, as a share of its maximum')
    p.add_argument('--png-encoder', dest='png_encoder', type=str, default='pillow', choices=['pillow', 'device'],
                   help='--mode infer into a PNG folder: pillow (default) encodes on writer threads with zlib; device '
                        'encodes on the GPU (DESIGN.md section 7i: Huffman-only deflate, larger files, no host codec on '
                        'the output side).  Not for y4m output')
    p.add_argument('--png-lz77', dest='png_lz77', action='store_true',
                   help='--png-encoder device: LZ77 matches inside every 32 KiB segment (DESIGN.md section 7n): smaller '
                        'files, never larger than without it, at a lower frame rate')
    p.add_argument('--output-size', dest='output_size', type=output_size_arg, default=None, metavar='WxH',
                   help='--mode infer: deliver every frame at W x H, resized on the GPU behind the generator (DESIGN.md '
                        'section 7j: antialiased bicubic, exact integers); each side within [1/4, 4] of the super-resolved '
                        'one, both even for y4m.  A y4m header gets the new size, and a pixel aspect ratio that keeps the '
                        'display aspect when the shape changes')
    p.add_argument('--deinterlace', dest='deinterlace', type=str, default='off', choices=['auto', 'off', 'tff', 'bff'],
                   help='y4m input: deinterlace on the GPU in front of the generator (DESIGN.md section 7o: edge-directed '
                        'line average bounded by a three-field motion measure; not compared with yadif or bwdif).  off: an '
                        "interlaced header is refused; auto: the header's field order, a progressive stream is left alone; "
                        'tff | bff: that field order whatever the header says')
    p.add_argument('--deinterlace-rate', dest='deinterlace_rate', type=str, default=None, choices=['field', 'frame'],
                   help='--deinterlace: field (default): two output frames per input frame and twice the frame rate in the '
                        "header; frame: the input's rate, the earlier field's frame only")
    p.add_argument('--raw-format', dest='raw_format', type=raw_format_arg, default=None, metavar='FMT',
                   help='--mode infer: the input (a file, or - for stdin) is headerless semi-planar raw video of this '
                        'format instead of y4m (DESIGN.md section 7p): nv12 nv16 nv24 p010 p012 p210 p212 p410 p412, '
                        "ffmpeg's -pix_fmt names; needs --raw-size")
    p.add_argument('--raw-size', dest='raw_size', type=output_size_arg, default=None, metavar='WxH',
                   help='--raw-format: the size of the frames')
    p.add_argument('--raw-rate', dest='raw_rate', type=raw_rate_arg, default=None, metavar='N:D',
                   help='--raw-format: frames per second, for the header of a y4m output (default 25:1)')
    p.add_argument('--output-format', dest='output_format', type=str, default=None, choices=['raw', 'y4m'],
                   help='y4m or raw input: what is written -- y4m (planar, with a header) or raw (headerless semi-planar '
                        'frames at --output-chroma / --output-depth; the format name and the size are printed on '
                        'stderr).  Default: raw for raw input, y4m for y4m input')
    args = p.parse_args(argv)
    if args.raw_format is not None and args.raw_size is None:
        p.error('--raw-format needs --raw-size WxH (headerless frames carry no size)')
    if args.raw_format is None and (args.raw_size is not None or args.raw_rate is not None):
        p.error('--raw-size and --raw-rate belong to --raw-format')
    if args.raw_format is not None and args.deinterlace != 'off':
        p.error('--deinterlace cannot be combined with --raw-format: interlaced semi-planar input is not supported '
                '(DESIGN.md section 7p)')
    y4m_input = bool(args.mode == 'infer' and args.input and (args.input == '-' or os.path.isfile(args.input)))
    if args.deinterlace != 'off' and not y4m_input:
        p.error('--deinterlace belongs to --mode infer with y4m input (a y4m file, or - for stdin)')
    if args.deinterlace_rate is not None and args.deinterlace == 'off':
        p.error('--deinterlace-rate belongs to --deinterlace auto|tff|bff')
    if args.output_size is not None and args.mode != 'infer':
        p.error('--output-size belongs to --mode infer')
    if args.output_depth is not None and not (args.mode == 'infer' and args.input and
                                              (args.input == '-' or os.path.isfile(args.input))):
        p.error('--output-depth belongs to --mode infer with y4m input (a y4m file, or - for stdin)')
    if args.output_chroma is not None and not (args.mode == 'infer' and args.input and
                                               (args.input == '-' or os.path.isfile(args.input))):
        p.error('--output-chroma belongs to --mode infer with y4m input (a y4m file, or - for stdin)')
    if args.output_depth not in (None, 8) and args.output_size is not None:
        p.error('--output-size resizes the 8-bit frames; it cannot be combined with --output-depth above 8')
    if args.png_encoder == 'device' and args.input and (args.input == '-' or os.path.isfile(args.input)):
        p.error('--png-encoder device writes PNG folders; y4m input is written as y4m')
    if (args.raw_format is not None or args.output_format is not None) and not y4m_input:
        p.error('--raw-format and --output-format belong to --mode infer with a file or - as the input')
    if args.png_lz77 and args.png_encoder != 'device':
        p.error('--png-lz77 belongs to --png-encoder device')
    return args


def default_opt():
    """The keys the hot path reads, with the shipped TecoGAN 4xSR BD values
    (experiments_BD/TecoGAN/TecoGAN_VimeoTecoGAN_4xSR_2GPU/train.yml) minus the VGG loss."""
    return {
        'scale': 4, 'manual_seed': 0,
        'dataset': {'degradation': {'type': 'BD', 'sigma': 1.5},
                    'train': {'crop_size': 128, 'batch_size_per_gpu': 2, 'tempo_extent': 10}},
        'model': {'name': 'TecoGAN',
                  'generator': {'name': 'FRNet', 'in_nc': 3, 'out_nc': 3, 'nf': 64, 'nb': 10},
                  'discriminator': {'name': 'STNet', 'in_nc': 3, 'tempo_range': 3}},
        'train': {'tempo_extent': 10, 'total_iter': 20,
                  'generator': {'lr': 5e-5, 'betas': [0.9, 0.999]},
                  'discriminator': {'update_policy': 'adaptive', 'update_threshold': 0.4,
                                    'crop_border_ratio': 0.75, 'lr': 5e-5, 'betas': [0.9, 0.999]},
                  'pixel_crit': {'type': 'CB', 'weight': 1, 'reduction': 'mean'},
                  'warping_crit': {'type': 'CB', 'weight': 1, 'reduction': 'mean'},
                  'pingpong_crit': {'type': 'CB', 'weight': 0.5, 'reduction': 'mean'},
                  'gan_crit': {'type': 'GAN', 'weight': 0.01, 'reduction': 'mean'}},
        'test': {'padding_mode': 'reflect', 'num_pad_front': 5},
        'logger': {'log_freq': 1, 'decay': 0.99, 'ckpt_freq': 0},
    }


def setup(args):
    if args.opt:
        with open(os.path.join(args.exp_dir, args.opt)) as f:
            opt = yaml.load(f.read(), Loader=yaml.FullLoader)
    else:
        opt = default_opt()
    opt['is_train'] = args.mode == 'train'
    if getattr(args, 'precision', None):
        opt['model']['generator']['precision'] = args.precision
    local_rank = int(os.environ.get('LOCAL_RANK', args.local_rank))
    if int(os.environ.get('WORLD_SIZE', '1')) > 1:
        dist_utils.init_dist(opt, max(local_rank, 0))
    else:
        if not torch.cuda.is_available():
            raise RuntimeError('an MI355X is required: the path has no CPU fallback')
        torch.cuda.set_device(int(args.gpu_ids.split(',')[0]))
        opt.update({'dist': False, 'device': 'cuda', 'rank': 0, 'world_size': 1})
    seed_everything(opt.get('manual_seed', 2021) + opt['rank'])          # base_utils.py:46
    if opt['is_train']:      # the reference's test.yml files have no `train` section
        opt['train'].setdefault('ckpt_dir', os.path.join(args.exp_dir, 'train', 'ckpt'))
    return opt


def seed_everything(seed):
    """setup_random_seed, base_utils.py:78-83: the LMDB data set draws its crop / flip / rotation /
    moving-first-frame geometry from Python's `random`, the degradation from numpy / torch."""
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)


def synthetic_train_batches(opt, n_iter, seed):
    """{'gt': n x t x 3 x (S+2b) x (S+2b) float32 in [0,1]} (BD: b = int(3 sigma); BI, degraded on the device: the
    bytes k / 255 a loader delivers, b = 2 scale)."""
    g = torch.Generator().manual_seed(seed)
    n = opt['dataset']['train'].get('batch_size_per_gpu', 2)
    t = opt['train']['tempo_extent']
    s = opt['dataset']['train']['crop_size']
    b = int(opt['dataset']['degradation'].get('sigma', 1.5) * 3.0)
    bi = opt['dataset']['degradation']['type'] == 'BI'
    if bi:
        b = 2 * opt['scale']
    for _ in range(n_iter):
        gt = torch.rand(n, t, 3, s + 2 * b, s + 2 * b, generator=g)
        yield {'gt': (gt * 255).round() / 255 if bi else gt}


def resume(model, opt, it):
    """Weights of iteration `it` + optimiser moments, schedule position and adaptive-D counter.
    The learning rate comes from the restored schedule position; every other hyper-parameter
    from the CURRENT yml."""
    ck = opt['train']['ckpt_dir']
    model.load_network(model.net_G, os.path.join(ck, f'G_iter{it}.pth'))
    if hasattr(model, 'net_D'):
        model.load_network(model.net_D, os.path.join(ck, f'D_iter{it}.pth'))
    got = model.resume_training_state(os.path.join(ck, f'state_iter{it}.pth'))
    if got != it:
        raise ValueError(f'state_iter{it}.pth was written at iteration {got}')
    return it


def train(opt, batches, start_iter=0):
    """codes/main.py:14-129 call sequence (logging to stdout on rank 0).  start_iter > 0:
    continue a checkpointed run (iterations are numbered from start_iter + 1, so checkpoints
    are not overwritten and the schedules continue where they stopped)."""
    model = define_model(opt)
    if start_iter:
        resume(model, opt, start_iter)
    for it, data in enumerate(batches, start_iter + 1):
        model.prepare_training_data(data)
        model.train()
        model.update_running_log()
        model.update_learning_rate()
        if opt['rank'] == 0 and it % opt['logger'].get('log_freq', 100) == 0:
            print(model.get_format_msg(0, it), flush=True)
        ck = opt['logger'].get('ckpt_freq', 0)
        if ck and it % ck == 0:
            os.makedirs(opt['train']['ckpt_dir'], exist_ok=True)
            model.save(it)
            model.save_training_state(it)      # optimiser moments etc.: restartable run
    return model


def test(opt, sequences, model_idx=None, ds_name=None):
    """codes/main.py:132-207: sequences sharded round-robin over ranks, PSNR-Y per sequence.
    `sequences`: list of {'gt': thwc uint8, 'lr': thwc float32, 'seq_idx': str}.
    With a `metric` section in opt the sequences are evaluated by MetricCalculator instead
    (evaluate(); it is returned)."""
    if opt.get('metric'):
        return evaluate(opt, sequences, model_idx or 'G_iter0', ds_name or 'test')
    model = define_model(opt)
    rank, world = dist_utils.get_dist_info()
    vals = [0.0] * len(sequences)
    for idx in dist_utils.shard_indices(len(sequences)):
        data = sequences[idx]
        model.prepare_inference_data(data)
        # output frames stay on the GPU; the GT clip goes up as raw uint8; the squared-error
        # sums come from the HIP kernel (metric_calculator.py:228-244 without the host trip)
        hr_seq = model.infer(device_output=True).contiguous()
        gt = data['gt'].to(hr_seq.device).contiguous()
        vals[idx] = float(np.mean(compute_psnr_device(gt, hr_seq)))      # (synchronises)
        model.net_G.check_faults()      # fail-safe of chained launches: the clip above is complete
    red = dist_utils.reduce_sum_to_master(vals, device=opt['device'] if opt['dist'] else 'cpu')
    if rank == 0:
        for d, v in zip(sequences, red.tolist()):
            print(f"{d['seq_idx']}: PSNR-Y {v:.3f} dB")
    return red


def evaluate(opt, sequences, model_idx, ds_name):
    """One model on one test set, as codes/main.py:158-205: infer each sequence (sharded over ranks),
    optionally save the frames (test.save_res / res_dir), compute the yml's metrics, gather them on
    rank 0 and write `{json_dir}/{ds_name}_avg.json` (test.save_json) or print them."""
    from .metrics.metric_calculator import MetricCalculator
    from .utils.data_utils import save_sequence
    model = define_model(opt)
    mc = MetricCalculator(opt)
    topt = opt.get('test', {})
    official = _official_metrics(opt) if topt.get('official_metrics') else None
    official_res = {}
    for idx in dist_utils.shard_indices(len(sequences)):
        data = sequences[idx]
        model.prepare_inference_data(data)
        hr_seq = model.infer(device_output=True).contiguous()
        mc.compute_sequence_metrics(data['seq_idx'], data['gt'], hr_seq)
        if official is not None:
            official_res[data['seq_idx']] = official.compute_sequence(data['gt'], hr_seq)
        model.net_G.check_faults()
        if topt.get('save_res'):
            res_dir = topt.get('res_dir') or os.path.join(opt.get('exp_dir', '.'), 'test', 'results')
            save_sequence(os.path.join(res_dir, ds_name, model_idx, data['seq_idx']), hr_seq.cpu().numpy(),
                          data.get('frm_idx'))
    seq_ids = getattr(sequences, 'keys', None) or [d['seq_idx'] for d in sequences]
    mc.gather(list(seq_ids))
    if topt.get('save_json'):
        json_dir = topt.get('json_dir') or os.path.join(opt.get('exp_dir', '.'), 'test', 'metrics')
        os.makedirs(json_dir, exist_ok=True)
        mc.save(model_idx, os.path.join(json_dir, f'{ds_name}_avg.json'), override=True)
    else:
        mc.display()
    if official is not None:
        _save_official(opt, official, official_res, list(seq_ids), model_idx, ds_name)
    return mc


def _official_metrics(opt):
    """test.official_metrics: the official protocol (metrics/official.py) next to the in-loop metrics.  Its LPIPS
    is a second instance WITH ScalingLayer, built from the weight paths of the metric section.  test.official_tof:
    true adds its tOF column (metrics/official.py)."""
    from .metrics.lpips import LPIPS
    from .metrics.official import OfficialMetrics
    device = opt.get('device', 'cuda')
    cfg = dict((opt.get('metric') or {}).get('LPIPS') or {})
    return OfficialMetrics(LPIPS.from_config(cfg, device=device, scaling=True), device=device,
                           tof=bool((opt.get('test') or {}).get('official_tof')))


def _save_official(opt, official, per_seq, seq_ids, model_idx, ds_name):
    """Ranks exchange per-sequence sums and counts; rank 0 writes `{json_dir}/{ds_name}_official.json`: the three
    aggregates, frame counts, crop windows, "skipped"; per-frame lists in the single-process case only."""
    import json
    from .metrics.official import reduce_and_aggregate, summary_lines
    rank, world = dist_utils.get_dist_info()
    dev = official.device if (opt.get('dist') and official.device.type == 'cuda') else 'cpu'
    agg = reduce_and_aggregate(per_seq, seq_ids, official.keys, device=dev)
    # windows and frame counts of the other ranks' sequences: 6 integers per sequence through the same reduction
    info = []
    for sid in seq_ids:
        r = per_seq.get(sid)
        info += ([r['frames'], r['evaluated']] + list(r['window'] or [0, 0, 0, 0])) if r else [0] * 6
    info = dist_utils.reduce_sum_to_master(info, device=dev).cpu().numpy().astype(np.int64).reshape(-1, 6)
    if rank != 0:
        return
    doc = {'model': model_idx, 'keys': list(official.keys), 'skipped': official.skipped, 'cutfr': official.cutfr,
           'sequences': list(seq_ids), 'frames': info[:, 0].tolist(), 'evaluated': info[:, 1].tolist(),
           'windows': info[:, 2:].tolist()}
    if official.tof:
        from .metrics.official import TOF_FLOW_NOTE
        doc['tOF_flow'] = TOF_FLOW_NOTE
    doc.update(agg)
    if world == 1:
        doc['per_frame'] = {sid: {k: per_seq[sid][k] for k in official.keys} for sid in seq_ids}
    topt = opt.get('test', {})
    json_dir = topt.get('json_dir') or os.path.join(opt.get('exp_dir', '.'), 'test', 'metrics')
    os.makedirs(json_dir, exist_ok=True)
    with open(os.path.join(json_dir, f'{ds_name}_official.json'), 'w') as f:
        json.dump(doc, f, indent=2)
    print('\n'.join(summary_lines(agg, official.keys)))


def folder_test_sets(opt):
    """[(name, FolderDataset)] of the yml's `dataset.test*` entries whose gt_seq_dir exists (sorted by
    entry name, as codes/main.py:154-158)."""
    from .data.folder_dataset import FolderDataset
    out = []
    deg = opt['dataset'].get('degradation', {}).get('type', 'BD')
    for key in sorted(opt.get('dataset', {})):
        d = opt['dataset'][key]
        if 'test' not in key or not isinstance(d, dict) or not d.get('gt_seq_dir'):
            continue
        if not os.path.isdir(d['gt_seq_dir']):
            continue
        if 'on_device' not in d and opt['dataset'].get('degradation', {}).get('on_device'):
            d = dict(d, on_device=True)         # BI without lr_seq_dir: LR from GT on the device
        out.append((d.get('name', key), FolderDataset(d, degradation=deg)))
    return out


# --mode infer: threads that copy a frame out of the stream's ring slot, encode and write it (PNG encoding releases the
# GIL).  A constant: the GPU boxes show hundreds of CPUs to a process that may use a few.
INFER_WRITER_THREADS = 4


def infer_sequences(input_dir):
    """[(sequence name, [frame paths])] of an --input folder: frames directly inside it are ONE sequence named ''
    (sub-folders are then ignored); otherwise every sub-folder that holds frames is a sequence (listed recursively and
    sorted, as folder_dataset.retrieve_files does)."""
    from .data.folder_dataset import retrieve_files
    names = sorted(os.listdir(input_dir))
    exts = ('.png', '.jpg')
    flat = [os.path.join(input_dir, n) for n in names
            if os.path.isfile(os.path.join(input_dir, n)) and os.path.splitext(n)[-1].lower() in exts]
    if flat:
        return [('', flat)]
    out = []
    for n in names:
        d = os.path.join(input_dir, n)
        if os.path.isdir(d):
            files = retrieve_files(d)
            if files:
                out.append((n, files))
    return out


def infer_output_path(input_dir, output_dir, seq, path):
    """Where the super-resolved frame of `path` goes: the input's name (and sub-folders) under output_dir, as .png."""
    rel = os.path.relpath(path, os.path.join(input_dir, seq) if seq else input_dir)
    return os.path.join(output_dir, seq, os.path.splitext(rel)[0] + '.png')


def scene_cut_option(args):
    """The SceneCut of --scene-cut [--scene-cut-mad X --scene-cut-hist Y], or None."""
    if not getattr(args, 'scene_cut', False):
        return None
    from .models.networks import SceneCut
    return SceneCut(mad=args.scene_cut_mad, hist=args.scene_cut_hist)


def log_scene_cuts(name, scene_cut):
    """The cut frames of one sequence, on stderr: stdout may be carrying the video."""
    import sys
    print(f'{name}: scene cuts at frames {scene_cut.cuts} (mad >= {scene_cut.mad:g}, hist >= {scene_cut.hist:g})',
          file=sys.stderr, flush=True)


def resize_option(output_size):
    """The Resize of --output-size WxH (as (w, h)), or None."""
    if output_size is None:
        return None
    from .models.networks import Resize
    return Resize(output_size[1], output_size[0])


def infer(opt, input_dir, output_dir, scene_cut=None, png_encoder='pillow', output_size=None, png_lz77=False):
    """--mode infer: every sequence of input_dir through VSRModel.infer_stream.  Frames are decoded one by one as the
    stream asks for them; the writers copy each frame out of the yielded ring slot before the generator is advanced.
    scene_cut (a SceneCut): passed on for every sequence, its cuts logged to stderr.  png_encoder 'device': the stream
    yields finished PNG files (infer_stream(png=Png())) and a writer copies one out of the slot and writes it as it
    is; 'pillow': the writers encode the RGB frames.  output_size (w, h): the frames are resized to it on the device
    (infer_stream(resize=Resize(h, w))), whichever encoder writes them.  png_lz77: the device encoder's LZ77 mode
    (Png(lz77=True)).  Returns {sequence: frames written}."""
    import threading
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image
    from .data.folder_dataset import read_rgb
    if png_encoder not in ('pillow', 'device'):
        raise ValueError(f"png_encoder is 'pillow' or 'device', got {png_encoder!r}")
    if png_lz77 and png_encoder != 'device':
        raise ValueError("png_lz77 belongs to png_encoder 'device'")
    seqs = infer_sequences(input_dir)
    if not seqs:
        raise ValueError(f'--input {input_dir}: no png | jpg frames, directly or one level down')
    model = define_model(opt)
    kw = {} if scene_cut is None else {'scene_cut': scene_cut}
    if png_encoder == 'device':
        from .models.networks import Png
        kw['png'] = Png(lz77=bool(png_lz77))
    if output_size is not None:
        kw['resize'] = resize_option(output_size)
    done = {}
    slots = threading.BoundedSemaphore(4 * INFER_WRITER_THREADS)       # frames copied out and not yet on disk

    def write(view, path, copied):
        try:
            try:
                frame = np.array(view)              # out of the ring slot
            finally:
                copied.release()
            os.makedirs(os.path.dirname(path), exist_ok=True)
            if png_encoder == 'device':             # the file as the GPU wrote it
                with open(path, 'wb') as f:
                    f.write(frame.data)
            else:
                Image.fromarray(frame).save(path)
        finally:
            slots.release()

    with ThreadPoolExecutor(max_workers=INFER_WRITER_THREADS) as pool:
        for seq, files in seqs:
            t0 = time.time()
            targets = [infer_output_path(input_dir, output_dir, seq, p) for p in files]
            jobs, k = [], 0
            for chunk in model.infer_stream((read_rgb(p) for p in files), **kw):
                copied = threading.Semaphore(0)
                for i in range(len(chunk)):
                    slots.acquire()
                    jobs.append(pool.submit(write, chunk[i], targets[k], copied))
                    k += 1
                for _ in range(len(chunk)):         # the slot is the generator's again once it is advanced
                    copied.acquire()
                running = []
                for j in jobs:                      # (the list does not grow with the clip; a writer's exception surfaces)
                    if j.done():
                        j.result()
                    else:
                        running.append(j)
                jobs = running
            for j in jobs:
                j.result()                          # (a writer's exception surfaces here)
            done[seq] = k
            if scene_cut is not None:
                log_scene_cuts(seq or os.path.basename(os.path.normpath(input_dir)), scene_cut)
            dt = time.time() - t0
            print(f"{seq or os.path.basename(os.path.normpath(input_dir))}: {k} frames -> "
                  f"{os.path.join(output_dir, seq)} ({k / max(dt, 1e-9):.1f} frames/s, bound by PNG decoding"
                  f"{' and writing' if png_encoder == 'device' else ' and encoding'})",
                  flush=True)
    model.net_G.check_faults()
    return done


def infer_y4m(opt, src, dst, matrix='bt709', yuv_range=None, scene_cut=None, output_size=None, siting='left',
              output_depth=None, output_chroma=None, deinterlace='off', deinterlace_rate=None, raw=None,
              output_format=None):
    """--mode infer on raw video: the y4m stream `src` (a binary file object) through VSRModel.infer_stream(yuv=...)
    into the y4m stream `dst`, in order.  The output header carries the scaled size and the input's F, A, C and X tags.
    Each chunk is written out of the ring slot before the generator is advanced; nothing is held beyond it.
    output_size (w, h): the frames are resized to it on the device; the header carries that size and, when the shape
    changes, an A tag scaled so that the display aspect stays.  The input may be C420p10 / C420p12 (DESIGN.md section
    7k): `siting` stands in where the header carries none.  output_depth 8 | 10 | 12 | None (the input's): bits per
    sample of the output; its C and XYSCSS tags follow.  The input may be C422 / C444 at any of the three depths, and
    output_chroma '420' | '422' | '444' | None (the input's) is the layout written; matrix may be
    'bt2020'.  A 4:2:0 clip with a 4:2:0 output and BT.601 / BT.709 runs as a Yuv420, everything else as a Yuv.
    deinterlace 'off' | 'auto' | 'tff' | 'bff' (DESIGN.md section 7o): with 'off' an It / Ib header is refused by the
    reader; 'auto' deinterlaces an It / Ib stream in the header's field order and leaves an Ip stream alone; 'tff' / 'bff'
    deinterlace in that order whatever the header says.  deinterlace_rate 'field' (None: the same) | 'frame': at field
    rate two frames are written per frame read and the header's F tag is doubled.  The header written says Ip.  Returns
    the number of frames written.
    raw (format, w, h, (rate n, d) | None): `src` is headerless semi-planar raw video instead (DESIGN.md section 7p;
    data/rawvideo.py), the range is `yuv_range` (None: limited) and the siting `siting`; not with deinterlace.
    output_format 'raw' | 'y4m' | None (raw for raw input, y4m for y4m input): 'raw' writes headerless semi-planar frames
    at output_chroma / output_depth and names their format and size on stderr; 'y4m' after raw input writes planar frames
    behind a header made from the size and the rate (25:1 without one).  Either input goes with either output."""
    import sys
    from .data.rawvideo import FORMAT_OF, RawReader, RawWriter
    from .data.y4m import TAG_OF_SITING, Y4MReader, Y4MWriter
    from .models.networks import Deinterlace, Yuv, Yuv420
    if deinterlace not in ('off', 'auto', 'tff', 'bff'):
        raise ValueError(f'deinterlace is off, auto, tff or bff, got {deinterlace!r}')
    if output_format not in (None, 'raw', 'y4m'):
        raise ValueError(f'output_format is raw, y4m or None, got {output_format!r}')
    raw_out = (raw is not None) if output_format is None else output_format == 'raw'
    if raw is not None:
        if deinterlace != 'off':
            raise ValueError('deinterlace cannot be combined with raw input: interlaced semi-planar input is not supported')
        fmt, rw, rh, rate = raw
        reader = RawReader(src, fmt, rw, rh)
        reader.siting, reader.full_range, reader.interlace = siting, None, 'p'
        tags = ['F%d:%d' % (rate or (25, 1)), 'C' + TAG_OF_SITING[siting]]
        if yuv_range is not None:                   # (a y4m written from it says what the command line said)
            tags.append('XCOLORRANGE=' + yuv_range.upper())
        reader.header = {'tags': tags, 'depth': reader.depth, 'chroma': reader.chroma}
    else:
        reader = Y4MReader(src, depths=(8, 10, 12), chromas=('420', '422', '444'), interlaced=deinterlace != 'off')
    order = {'t': 'tff', 'b': 'bff', 'p': None}[reader.interlace] if deinterlace == 'auto' else \
        None if deinterlace == 'off' else deinterlace
    deint = None if order is None else Deinterlace(tff=order == 'tff', rate=deinterlace_rate or 'field')
    full = reader.full_range if yuv_range is None else yuv_range == 'full'
    common = dict(matrix=matrix, full_range=bool(full), siting=reader.siting if reader.siting is not None else siting,
                  depth=reader.depth, out_depth=output_depth)
    if raw is not None or raw_out:
        spec = Yuv(reader.h, reader.w, chroma=reader.chroma, out_chroma=output_chroma, **common,
                   layout='planar' if raw is None else 'semi', out_layout='semi' if raw_out else 'planar')
        oc = spec.oc
    elif reader.chroma == '420' and output_chroma in (None, '420') and matrix != 'bt2020':
        spec, oc = Yuv420(reader.h, reader.w, **common), '420'
    else:
        spec = Yuv(reader.h, reader.w, chroma=reader.chroma, out_chroma=output_chroma, **common)
        oc = spec.oc
    model = define_model(opt)
    s = model.net_G.scale
    W, H = s * reader.w, s * reader.h
    kw = {} if scene_cut is None else {'scene_cut': scene_cut}
    if deint is not None:
        deint.check_source(spec)
        kw['deinterlace'] = deint
    aspect = None
    if output_size is not None:
        ow, oh = output_size
        if oc == '420' and (ow % 2 or oh % 2):
            raise ValueError(f'--output-size {ow}x{oh}: a 4:2:0 frame has even sides')
        if oc == '422' and ow % 2:
            raise ValueError(f'--output-size {ow}x{oh}: a 4:2:2 frame has an even width')
        kw['resize'] = resize_option(output_size)
        kw['resize'].check_source(H, W)
        if oh * W != ow * H:                        # the shape changes: every pixel becomes this much wider for its height
            aspect = (W * oh, H * ow)
        W, H = ow, oh
    if raw_out:
        writer = RawWriter(dst, spec.out_size_bytes(H, W))
        print(f'raw: writing {FORMAT_OF[(oc, spec.od)]} {W}x{H} (ffmpeg -f rawvideo -pix_fmt {FORMAT_OF[(oc, spec.od)]}'
              f'{"le" if spec.od > 8 else ""} -s {W}x{H})', file=sys.stderr, flush=True)
    else:
        writer = Y4MWriter(dst, W, H, reader.header, aspect_scale=aspect, depth=spec.od, siting=spec.siting, chroma=oc,
                           rate_scale=(2, 1) if deint is not None and deint.rate == 'field' else None)
    t0, k = time.time(), 0
    for chunk in model.infer_stream(reader, yuv=spec, **kw):
        for frame in chunk:
            writer.write(frame)
            k += 1
    writer.flush()
    model.net_G.check_faults()
    if scene_cut is not None:
        log_scene_cuts('y4m', scene_cut)
    dt = time.time() - t0
    print(f'{"y4m" if raw is None else raw[0]}: {k} frames {reader.w}x{reader.h} -> {W}x{H} '
          f'({k / max(dt, 1e-9):.1f} frames/s, {spec.matrix} {"full" if spec.full_range else "limited"} range, '
          f'{spec.siting} siting, {spec.depth} -> {spec.od} bits, {reader.chroma} -> {oc})', flush=True)
    if deinterlace != 'off':
        print(f'y4m: deinterlace {deinterlace}: {reader.frames_read} frames in, {k} frames out, '
              + ('progressive input left alone' if deint is None else f'{order} at {deint.rate} rate'),
              file=sys.stderr, flush=True)
    return k


def infer_y4m_cli(opt, input_path, output_path, matrix, yuv_range, scene_cut=None, output_size=None, siting='left',
                  output_depth=None, output_chroma=None, deinterlace='off', deinterlace_rate=None, raw=None,
                  output_format=None):
    """Opens the two ends of infer_y4m.  With `--output -` the y4m bytes are the ONLY thing on stdout: the descriptor
    is set aside for them and, for the length of the run, descriptor 1 and sys.stdout lead to stderr, so that neither
    a print nor a library's message can land in the stream."""
    import sys
    src = sys.stdin.buffer if input_path == '-' else open(input_path, 'rb')
    try:
        if output_path != '-':
            with open(output_path, 'wb') as dst:
                return infer_y4m(opt, src, dst, matrix, yuv_range, scene_cut, output_size, siting, output_depth,
                                 output_chroma, deinterlace, deinterlace_rate, raw, output_format)
        sys.stdout.flush()
        keep = os.dup(1)
        py_stdout = sys.stdout
        os.dup2(2, 1)
        sys.stdout = sys.stderr
        try:
            with os.fdopen(os.dup(keep), 'wb') as dst:
                return infer_y4m(opt, src, dst, matrix, yuv_range, scene_cut, output_size, siting, output_depth,
                                 output_chroma, deinterlace, deinterlace_rate, raw, output_format)
        finally:
            sys.stdout = py_stdout
            os.dup2(keep, 1)
            os.close(keep)
    finally:
        if src is not sys.stdin.buffer:
            src.close()


def profile(opt, lr_size, test_speed=False):
    """codes/main.py:210-264 protocol: FLOPs/params, then FPS of step() over 30 fresh random
    inputs with a device sync per frame."""
    device = torch.device('cuda')
    net_G = define_generator(opt).to(device)
    gflops, params = net_G.profile(lr_size, device)
    for k in gflops:
        print(f'{k}: {gflops[k]:.3f} GFLOPs, {params[k] / 1e6:.3f} M params')
    print(f'total: {sum(gflops.values()):.3f} GFLOPs, {sum(params.values()) / 1e6:.3f} M params')
    if not test_speed:
        return None
    net_G.eval()
    n_test, tot = 30, 0.0
    with torch.no_grad():
        for _ in range(n_test):
            dummy = net_G.generate_dummy_data(lr_size, device)
            torch.cuda.synchronize()
            t0 = time.time()
            net_G.step(*dummy)
            torch.cuda.synchronize()
            tot += time.time() - t0
    fps = n_test / tot
    print(f'Speed: {fps:.2f} FPS ({1e3 * tot / n_test:.3f} ms/frame)')
    return fps


def main(argv=None):
    args = parse_args(argv)
    opt = setup(args)
    if args.mode == 'train' and opt['dataset'].get('train', {}).get('seq_dir') and \
            os.path.exists(opt['dataset']['train']['seq_dir']):
        from .data import TrainSource
        src = TrainSource(opt)

        total = int(opt['train'].get('total_iter', 0))
        n_iter = args.iters if args.iters is not None else max(0, total - args.resume)
        per_epoch = max(1, len(src))
        # a resumed run continues in the epoch (and at the batch) iteration `resume` had reached:
        # the sampler order of an epoch is a function of (seed, epoch) alone
        ep0, skip = divmod(args.resume, per_epoch)
        if ep0 > 0:
            src.replay(ep0)      # the geometry draws of the finished epochs (random streams aligned with an uninterrupted run)

        def epochs():
            ep, left, sk = ep0, n_iter, skip
            while left > 0:
                for i, b in enumerate(src.epoch(ep, first_batch=sk)):
                    if left <= 0:
                        return
                    left -= 1
                    yield b
                ep, sk = ep + 1, 0
        train(opt, epochs(), start_iter=args.resume)
    elif args.mode == 'train':
        train(opt, synthetic_train_batches(opt, 20 if args.iters is None else args.iters,
                                           100 + opt['rank'] + 7919 * args.resume),
              start_iter=args.resume)
    elif args.mode == 'test' and folder_test_sets(opt):
        opt['exp_dir'] = args.exp_dir
        gen = opt['model']['generator']
        model_idx = os.path.splitext(os.path.basename(gen['load_path']))[0] if gen.get('load_path') else 'G_iter0'
        for ds_name, seqs in folder_test_sets(opt):
            test(opt, seqs, model_idx=model_idx, ds_name=ds_name)
    elif args.mode == 'test':
        g = torch.Generator().manual_seed(7)
        seqs = []
        for i in range(4):
            lr = torch.rand(8, 32, 48, 3, generator=g)
            gt = (torch.rand(8, 32 * opt['scale'], 48 * opt['scale'], 3, generator=g) * 255).to(torch.uint8)
            seqs.append({'gt': gt, 'lr': lr, 'seq_idx': f'synthetic_{i:03d}'})
        test(opt, seqs)
    elif args.mode == 'infer':
        if not args.input or not args.output:
            raise ValueError('--mode infer needs --input DIR and --output DIR (or a y4m file / - for both)')
        if args.input == '-' or os.path.isfile(args.input):
            infer_y4m_cli(opt, args.input, args.output, args.yuv_matrix, args.yuv_range, scene_cut_option(args),
                          args.output_size, args.yuv_siting, args.output_depth, args.output_chroma, args.deinterlace,
                          args.deinterlace_rate,
                          None if args.raw_format is None else (args.raw_format, *args.raw_size, args.raw_rate),
                          args.output_format)
        else:
            infer(opt, args.input, args.output, scene_cut_option(args), args.png_encoder, args.output_size, args.png_lz77)
    elif args.mode == 'profile':
        profile(opt, tuple(int(v) for v in args.lr_size.split('x')), args.test_speed)
    else:
        raise ValueError(f'Unrecognized mode: {args.mode} (train|test|profile|infer)')


if __name__ == '__main__':
    main()
