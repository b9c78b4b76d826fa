"""GPU: the BI degradation (tg_downsample_bi_u8 / _f32, ops.downsample_bi) BIT FOR BIT against
the integer specification tests/bi_ref.py -- at sizes that take every path of the kernel (dword and byte staging,
partial tiles, a halo that wraps more than once, modcrop), in every form (pad, input type, outputs) -- and the
wiring: test mode without LR frames against the frames make_lr writes, on-device BI training batches."""
import os
import pickle

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import bi_ref as R
from tecogan_pytorch_amd import _lib as L
from tecogan_pytorch_amd import ops

DEV = 'cuda'
TH, TW = ops.BI_TILE


def _sizes(s):
    assert (67 * s // s) % TH and (131 * s // s) % TW          # no multiple of the tile in either axis
    return [(s, 2 * s),                   # one LR row; the halo wraps twice
            (4 * s + 3, 5 * s + 1),       # modcrop
            (67 * s, 131 * s),            # several tiles per axis, partial ones at both ends
            (5 * s + 1, 132 * s),         # rows of 3W bytes keep one dword alignment: dword staging inside
            (3 * s, 70 * s + 2)]          # ... and do not: byte staging everywhere


_REF = {}


def _case(s, size, n):
    """Input and expected bytes, made once per case and shared."""
    key = (s, size, n)
    if key not in _REF:
        rs = np.random.RandomState(1000 * s + size[0] + 7 * size[1] + n)
        x = rs.randint(0, 256, (n,) + size + (3,)).astype(np.uint8)
        x[0, : size[0] // 2] = (x[0, : size[0] // 2] > 127) * 255             # {0, 255}: both clamps
        _REF[key] = (x, R.bi_downsample_u8(x, s, pad=True))
    return _REF[key]


def _check(got8, got32, ref8, what):
    if got8 is not None:
        assert got8.dtype == torch.uint8 and tuple(got8.shape) == ref8.shape, what
        assert np.array_equal(got8.cpu().numpy(), ref8), what
    if got32 is not None:
        assert got32.dtype == torch.float32
        assert torch.equal(got32.cpu(), torch.from_numpy(R.bi_lr_float(ref8))), what


@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('size_idx', range(5))
@pytest.mark.parametrize('s', [2, 4])
def test_bytes_equal_the_specification(s, size_idx, n):
    size = _sizes(s)[size_idx]
    x, ref = _case(s, size, n)
    xu = torch.from_numpy(x).to(DEV)
    xf = ops.dequantize_u8_hwc(xu)                                  # k / 255, fp32 NCHW: what the loaders deliver
    hc, wc = size[0] - size[0] % s, size[1] - size[1] % s
    for pad in (True, False):
        if not pad and not (hc > 4 * s and wc > 4 * s):
            for inp in (xu, xf):
                with pytest.raises(L.TecoganHipError):
                    ops.downsample_bi(inp, s, pad=False)
            continue
        want = ref if pad else np.ascontiguousarray(ref[:, 2:-2, 2:-2])
        if not pad:
            assert np.array_equal(want, R.bi_downsample_u8(x, s, pad=False))
        for name, inp in (('u8', xu), ('f32', xf)):
            y32, y8 = ops.downsample_bi(inp, s, pad=pad, out='both')
            _check(y8, y32, want, (s, size, n, pad, name, 'both'))
            _check(ops.downsample_bi(inp, s, pad=pad, out='u8'), None, want, (s, size, n, pad, name, 'u8'))
            _check(None, ops.downsample_bi(inp, s, pad=pad), want, (s, size, n, pad, name, 'f32'))


@pytest.mark.parametrize('s', [2, 4])
def test_all_256_bytes(s):
    """The weights sum to 1: a constant frame of value k gives k everywhere, as byte and as (float)k / 255 -- all 256
    in one launch; and 256 constant bands of 4s columns against the specification."""
    x = np.broadcast_to(np.arange(256, dtype=np.uint8)[:, None, None, None], (256, 2 * s, 3 * s, 3)).copy()
    y32, y8 = ops.downsample_bi(torch.from_numpy(x).to(DEV), s, out='both')
    k = torch.arange(256, dtype=torch.uint8)
    assert torch.equal(y8.cpu(), k[:, None, None, None].expand(256, 2, 3, 3))
    assert torch.equal(y32.cpu(), (k.float() / 255.0)[:, None, None, None].expand(256, 3, 2, 3))
    y32f = ops.downsample_bi(ops.dequantize_u8_hwc(torch.from_numpy(x).to(DEV)), s)
    assert torch.equal(y32f, y32)
    bands = np.repeat(np.arange(256, dtype=np.uint8), 4 * s)[None, None, :, None]
    bands = np.ascontiguousarray(np.broadcast_to(bands, (1, 2 * s, 256 * 4 * s, 3)))
    ref = R.bi_downsample_u8(bands, s)
    assert len(np.unique(ref)) == 256
    y32, y8 = ops.downsample_bi(torch.from_numpy(bands).to(DEV), s, out='both')
    _check(y8, y32, ref, ('bands', s))


@pytest.mark.parametrize('s', [2, 4])
def test_accumulator_width(s):
    """x = 255 where kv[r] * kh[c] > 0, period 4s, in phase with every fourth LR pixel: for s = 4 the exact sum there is
    255 * (4448^2 + 352^2) > 2^32 (a 32-bit accumulate would wrap to a small byte); the specification clamps to 255."""
    k = R.WEIGHTS[s]
    T = 4 * s
    idx = (np.arange(3 * T) + 3 * s // 2) % T
    pat = ((np.outer(k[idx], k[idx]) > 0) * 255).astype(np.uint8)
    x = np.ascontiguousarray(np.broadcast_to(pat[None, :, :, None], (1, 3 * T, 3 * T, 3)))
    N = R.exact_sums(x, s)
    pos, neg = int(k[k > 0].sum()), int(-k[k < 0].sum())
    assert int(N[0, 4, 4, 0]) == 255 * (pos * pos + neg * neg)
    if s == 4:
        assert int(N[0, 4, 4, 0]) > 2 ** 32
    ref = R.bi_downsample_u8(x, s)
    assert ref[0, 4, 4, 0] == 255 and ref.min() == 0
    xu = torch.from_numpy(x).to(DEV)
    for inp in (xu, ops.dequantize_u8_hwc(xu)):
        y32, y8 = ops.downsample_bi(inp, s, out='both')
        _check(y8, y32, ref, ('accumulator', s))


def test_argument_checks():
    lib = L.lib()
    x = torch.zeros(1, 16, 16, 3, dtype=torch.uint8, device=DEV)
    y = torch.zeros(1, 8, 8, 3, dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    assert lib.tg_downsample_bi_u8(x.data_ptr(), y.data_ptr(), None, 1, 16, 16, 3, 1, st) == -2       # scale
    assert lib.tg_downsample_bi_u8(x.data_ptr(), None, None, 1, 16, 16, 2, 1, st) == -2               # no output
    assert lib.tg_downsample_bi_u8(x.data_ptr(), y.data_ptr(), None, 1, 1, 16, 2, 1, st) == -1        # smaller than a block
    assert lib.tg_downsample_bi_u8(x.data_ptr(), y.data_ptr(), None, 1, 16, 16, 4, 0, st) == -1       # pad=0: 16 <= 4s
    assert lib.tg_downsample_bi_f32(None, y.data_ptr(), None, 1, 16, 16, 2, 1, st) == -2
    for bad in (x.cpu(), x.float(), x.permute(0, 3, 1, 2)):
        with pytest.raises(L.TecoganHipError):
            ops.downsample_bi(bad, 2)
    with pytest.raises(L.TecoganHipError):
        ops.downsample_bi(x, 2, out='f16')


# ---------------------------------------------------------------------------------------------------------- wiring
def _test_opt(scale):
    return {'scale': scale, 'dist': False, 'device': 'cuda', 'rank': 0, 'world_size': 1, 'is_train': False,
            'dataset': {'degradation': {'type': 'BI'}},
            'model': {'name': 'FRVSR', 'generator': {'name': 'FRNet', 'in_nc': 3, 'out_nc': 3, 'nf': 64, 'nb': 10,
                                                     'load_path': None}},
            'test': {'padding_mode': 'reflect', 'num_pad_front': 1}}


def test_test_mode_without_lr_equals_the_frames_make_lr_wrote(tmp_path):
    """2xBI end to end: a BI FolderDataset without lr_seq_dir (`on_device`: LR made by prepare_inference_data) gives
    the same uint8 output frames as one whose lr_seq_dir holds the PNGs make_lr wrote from the same GT."""
    from PIL import Image
    from procedural_weights import generator_state_dict
    from tecogan_pytorch_amd.data import make_lr
    from tecogan_pytorch_amd.data.folder_dataset import FolderDataset, read_rgb
    from tecogan_pytorch_amd.models import define_model
    s = 2
    rs = np.random.RandomState(9)
    gts = {}
    for key in ('calendar', 'city'):
        (tmp_path / 'gt' / key).mkdir(parents=True)
        for i in range(3):
            img = rs.randint(0, 256, (32, 48, 3)).astype(np.uint8)
            Image.fromarray(img).save(str(tmp_path / 'gt' / key / f'{i:04d}.png'))
            gts[(key, i)] = img
    done = make_lr.main(['--gt', str(tmp_path / 'gt'), '--out', str(tmp_path / 'lr'), '--degradation', 'BI',
                         '--scale', str(s)])
    assert done == 0
    for (key, i), img in gts.items():                                   # the tool writes the specification's bytes
        assert np.array_equal(read_rgb(str(tmp_path / 'lr' / key / f'{i:04d}.png')), R.bi_downsample_u8(img, s))
    opt = _test_opt(s)
    m = define_model(opt)
    m.net_G.load_state_dict(generator_state_dict(scale=s, degradation='BI'), strict=True)
    alone = FolderDataset({'gt_seq_dir': str(tmp_path / 'gt'), 'on_device': True}, degradation='BI')
    paired = FolderDataset({'gt_seq_dir': str(tmp_path / 'gt'), 'lr_seq_dir': str(tmp_path / 'lr')}, degradation='BI')
    assert alone.keys == paired.keys == ['calendar', 'city']
    for a, p in zip(alone, paired):
        assert 'lr' not in a and 'lr' in p
        m.prepare_inference_data(a)
        lr_a = m.lr_data.cpu()
        hr_a = m.infer()
        m.prepare_inference_data(p)
        assert torch.equal(lr_a, m.lr_data.cpu())
        hr_p = m.infer()
        assert hr_a.dtype == np.uint8 and hr_a.shape == (3, 32, 48, 3) and np.array_equal(hr_a, hr_p)
    m.net_G.check_faults()


def test_make_lr_bd_writes_the_quantised_device_degradation(tmp_path):
    from PIL import Image
    from tecogan_pytorch_amd.data import make_lr
    from tecogan_pytorch_amd.data.folder_dataset import read_rgb
    from tecogan_pytorch_amd.utils.data_utils import gaussian_kernel2d
    rs = np.random.RandomState(10)
    (tmp_path / 'gt' / 'a' / 'sub').mkdir(parents=True)
    img = rs.randint(0, 256, (24, 36, 3)).astype(np.uint8)
    Image.fromarray(img).save(str(tmp_path / 'gt' / 'a' / 'sub' / 'f.png'))
    assert make_lr.make_lr(str(tmp_path / 'gt'), str(tmp_path / 'lr'), 'BD', 4, sigma=1.5) == {'a': 1}
    lr = ops.downsample_bd(ops.dequantize_u8_hwc(torch.from_numpy(img[None]).to(DEV)), gaussian_kernel2d(1.5), 4, True)
    want = ops.quantize_u8_hwc(lr[0]).cpu().numpy()
    assert np.array_equal(read_rgb(str(tmp_path / 'lr' / 'a' / 'sub' / 'f.png')), want)      # layout mirrored


def test_on_device_bi_training_batches(tmp_path):
    """dataset.degradation {type: BI, on_device: true}: unpaired GT crops of crop_size + 4 * scale; LR = the
    specification applied to the gathered crop, GT = its centre; one training step runs.  Without the key the paired
    branch is still chosen."""
    from tests.test_hip_train import make_opt
    from tecogan_pytorch_amd.data import LMDBWriter, PairedLMDBDataset, TrainSource, UnpairedLMDBDataset
    from tecogan_pytorch_amd.models import define_model
    from tests.test_data_cpu import _make_paired_envs
    s, crop, t = 4, 32, 3
    rs = np.random.RandomState(11)
    frames = {f'clip_000_5x52x60_{i:04d}': rs.randint(0, 256, (52, 60, 3)).astype(np.uint8) for i in range(5)}
    env = tmp_path / 'gt_lmdb'
    LMDBWriter(str(env)).write({k: v.tobytes() for k, v in frames.items()})
    with open(os.path.join(str(env), 'meta_info.pkl'), 'wb') as f:
        pickle.dump({'name': 'bi', 'color': 'RGB', 'keys': list(frames.keys())}, f)
    opt = make_opt('FRVSR')
    opt['scale'] = s
    opt['dataset']['degradation'] = {'type': 'BI', 'on_device': True}
    opt['dataset']['train'].update({'seq_dir': str(env), 'filter_file': None, 'data_type': 'rgb', 'crop_size': crop,
                                    'batch_size_per_gpu': 2})
    opt['train']['tempo_extent'] = t
    src = TrainSource(opt)
    assert isinstance(src.dataset, UnpairedLMDBDataset) and not src.paired and src.dataset.crop_size == crop + 4 * s
    b = next(iter(src.epoch(0)))
    assert set(b) == {'gt'} and tuple(b['gt'].shape) == (2, t, 3, crop + 4 * s, crop + 4 * s) and b['gt'].is_cuda
    m = define_model(opt)
    m.prepare_training_data(b)
    gt_u8 = (b['gt'].cpu() * 255.0).round().to(torch.uint8)
    assert torch.equal(gt_u8.float() / 255.0, b['gt'].cpu())                         # the gather delivers k / 255
    hwc = gt_u8.permute(0, 1, 3, 4, 2).contiguous().numpy()
    want_lr = R.bi_lr_float(R.bi_downsample_u8(hwc, s, pad=False))
    assert tuple(m.lr_data.shape) == (2, t, 3, crop // s, crop // s)
    assert torch.equal(m.lr_data.cpu(), torch.from_numpy(want_lr))
    assert torch.equal(m.gt_data.cpu(), b['gt'].cpu()[..., 2 * s:2 * s + crop, 2 * s:2 * s + crop])
    m.train()
    assert np.isfinite(m.log_dict['l_pix_G'])
    # without on_device: the paired sets, as before
    gt_dir, lr_dir = _make_paired_envs(tmp_path / 'paired')
    opt2 = make_opt('FRVSR')
    opt2['scale'] = 2
    opt2['dataset']['degradation'] = {'type': 'BI'}
    opt2['dataset']['train'].update({'gt_seq_dir': gt_dir, 'lr_seq_dir': lr_dir, 'filter_file': None,
                                     'data_type': 'rgb', 'gt_crop_size': 16, 'batch_size_per_gpu': 2, 'name': 'REDS'})
    opt2['train']['tempo_extent'] = 4
    src2 = TrainSource(opt2)
    assert isinstance(src2.dataset, PairedLMDBDataset) and src2.paired
