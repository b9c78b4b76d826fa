"""CPU: the BI degradation's specification (tests/bi_ref.py) pinned independently of the kernel:
the integer tables against MATLAB's contribution algorithm in fp64, the integer route against the fp64 route and
against torch's antialiased bicubic in the interior, and the host-side wiring (FolderDataset, make_lr's flags)."""
import os
import re

import numpy as np
import pytest
import torch

from tests import bi_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIE_SHARE = 1e-3          # at most 0.1 % of the pixels may sit on an exact tie (left out of the comparisons)


@pytest.mark.parametrize('s', [2, 4])
def test_weight_tables_are_matlabs_contributions(s):
    k, den = R.WEIGHTS[s], R.DENOM[s]
    assert k.shape == (4 * s,) and int(k.sum()) == den and np.array_equal(k, k[::-1])
    assert int(np.abs(k).sum()) == {2: 304, 4: 4800}[s]
    for n in (s, 2 * s, 3 * s, 7 * s, 12 * s, 16 * s, 67 * s):
        w, idx = R.matlab_contributions(n, n // s, 1.0 / s)
        assert w.shape == (n // s, 4 * s)
        scaled = w * den
        assert np.array_equal(scaled, np.tile(k.astype(np.float64), (n // s, 1))), n      # exactly, every row alike
        assert np.array_equal(scaled.sum(axis=1), np.full(n // s, float(den)))
        assert np.array_equal(idx, R.tap_indices(n, s)), n                                  # incl. the multi-wrap halo
    # the mirror repeats the edge pixel (numpy's 'symmetric'), not 'reflect'
    assert R.mirror_index([-1, -2, 5, 6, -7, 12], 5).tolist() == [0, 1, 4, 3, 3, 2]


def _shapes(s):
    return [(12 * s, 16 * s), (s, 2 * s), (4 * s + 3, 5 * s + 1)]


@pytest.mark.parametrize('s', [2, 4])
def test_integer_route_equals_fp64_route(s):
    rs = np.random.RandomState(50 + s)
    for shape in _shapes(s):
        for kind in ('uniform', 'binary'):
            x = rs.randint(0, 256, shape + (3,)).astype(np.uint8)
            if kind == 'binary':
                x = (x > 127).astype(np.uint8) * 255                  # both clamps
            N = R.exact_sums(x, s)
            tie = R.is_tie(N, s)                                      # from the integers alone
            assert tie.mean() <= TIE_SHARE
            got, ref = R.bi_downsample_u8(x, s), R.bi_downsample_fp64(x, s)
            assert got.shape == (shape[0] // s, shape[1] // s, 3) and got.dtype == np.uint8
            assert np.array_equal(got[~tie], ref[~tie]), (shape, kind)
    # batched input = frame by frame
    xb = rs.randint(0, 256, (2, 3, 5 * s, 6 * s, 3)).astype(np.uint8)
    yb = R.bi_downsample_u8(xb, s)
    assert np.array_equal(yb[1, 2], R.bi_downsample_u8(xb[1, 2], s))


@pytest.mark.parametrize('s', [2, 4])
def test_interior_equals_torch_antialiased_bicubic(s):
    """An independent implementation of the same kernel (a = -0.5, stretched by s): away from the borders, which it
    treats differently, its rounded bytes are the specification's."""
    rs = np.random.RandomState(60 + s)
    x = rs.randint(0, 256, (12 * s, 16 * s, 3)).astype(np.uint8)
    t = torch.from_numpy(x.astype(np.float64) / 255.0).permute(2, 0, 1)[None]
    y = torch.nn.functional.interpolate(t, scale_factor=1.0 / s, mode='bicubic', antialias=True, align_corners=False)
    ref = np.floor(np.clip(y[0].permute(1, 2, 0).numpy(), 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)
    got = R.bi_downsample_u8(x, s)
    tie = R.is_tie(R.exact_sums(x, s), s)
    assert tie.mean() <= TIE_SHARE
    inner = np.zeros(got.shape, dtype=bool)
    inner[2:-2, 2:-2] = True
    keep = inner & ~tie
    assert keep.sum() >= 0.5 * got.size and np.array_equal(got[keep], ref[keep])


@pytest.mark.parametrize('s', [2, 4])
def test_pad_false_is_the_cut_pad_true_result(s):
    rs = np.random.RandomState(70 + s)
    x = rs.randint(0, 256, (2, 4 * s + 3 * s, 4 * s + s + 1, 3)).astype(np.uint8)
    full, cut = R.bi_downsample_u8(x, s, pad=True), R.bi_downsample_u8(x, s, pad=False)
    assert cut.shape == (2, 3, 1, 3) and np.array_equal(cut, full[:, 2:-2, 2:-2])
    with pytest.raises(ValueError):
        R.bi_downsample_u8(x[:, :4 * s], s, pad=False)
    with pytest.raises(ValueError):
        R.bi_downsample_u8(x, 3)
    # a constant image stays constant (the weights sum to 1)
    for k in (0, 1, 127, 128, 254, 255):
        assert np.all(R.bi_downsample_u8(np.full((3 * s, 5 * s, 3), k, np.uint8), s) == k)
    f = R.bi_lr_float(full)
    assert f.dtype == np.float32 and f.shape == (2, 3) + full.shape[1:3]
    assert np.array_equal(f[1, 2], full[1, :, :, 2].astype(np.float32) / np.float32(255))


def test_folder_dataset_bi_without_lr_yields_gt_only(tmp_path):
    from PIL import Image
    from tecogan_pytorch_amd.data.folder_dataset import FolderDataset
    rs = np.random.RandomState(3)
    for key in ('a', 'b'):
        (tmp_path / 'gt' / key).mkdir(parents=True)
        for i in range(2):
            Image.fromarray(rs.randint(0, 256, (8, 12, 3)).astype(np.uint8)).save(str(tmp_path / 'gt' / key / f'{i:04d}.png'))
    ds = FolderDataset({'gt_seq_dir': str(tmp_path / 'gt'), 'on_device': True}, degradation='BI')
    assert ds.keys == ['a', 'b']
    d = ds[0]
    assert 'lr' not in d and d['gt'].dtype == torch.uint8 and tuple(d['gt'].shape) == (2, 8, 12, 3)
    assert d['frm_idx'] == ['0000.png', '0001.png']
    with pytest.raises(ValueError, match='on_device'):             # paired unless the entry opts in
        FolderDataset({'gt_seq_dir': str(tmp_path / 'gt')}, degradation='BI')
    # main.folder_test_sets hands dataset.degradation.on_device down to the entries
    from tecogan_pytorch_amd.main import folder_test_sets
    opt = {'dataset': {'degradation': {'type': 'BI', 'on_device': True}, 'test1': {'gt_seq_dir': str(tmp_path / 'gt')}}}
    (name, got), = folder_test_sets(opt)
    assert name == 'test1' and got.keys == ['a', 'b'] and 'lr' not in got[1]
    opt['dataset']['degradation'] = {'type': 'BI'}
    with pytest.raises(ValueError):
        folder_test_sets(opt)


def test_make_lr_flags():
    from tecogan_pytorch_amd.data import make_lr
    a = make_lr.parse_args(['--gt', 'g', '--out', 'o', '--degradation', 'BI', '--scale', '2'])
    assert (a.gt, a.out, a.degradation, a.scale, a.sigma) == ('g', 'o', 'BI', 2, 1.5)
    a = make_lr.parse_args(['--gt', 'g', '--out', 'o', '--degradation', 'BD', '--scale', '4', '--sigma', '1.2'])
    assert (a.degradation, a.scale, a.sigma) == ('BD', 4, 1.2)
    for bad in (['--scale', '3', '--degradation', 'BI'], ['--scale', '4', '--degradation', 'XX'], ['--scale', '4']):
        with pytest.raises(SystemExit):
            make_lr.parse_args(['--gt', 'g', '--out', 'o'] + bad)
    with pytest.raises(ValueError):
        make_lr.make_lr('g', 'o', 'BI', 3)


def test_tile_constant_and_tables_agree_with_the_sources():
    """ops.BI_TILE mirrors the header's TG_BI_TILE_*; the kernel's weight tables are the specification's."""
    from tecogan_pytorch_amd import ops
    head = open(os.path.join(ROOT, 'include', 'tecogan_hip.h')).read()
    th = int(re.search(r'#define TG_BI_TILE_H (\d+)', head).group(1))
    tw = int(re.search(r'#define TG_BI_TILE_W (\d+)', head).group(1))
    assert ops.BI_TILE == (th, tw) and ops.BI_BORDER_LR == R.BORDER_LR
    src = open(os.path.join(ROOT, 'tecogan-pytorch_amd', 'csrc', 'tg_resize.hip')).read()
    for s, name in ((2, 'h2'), (4, 'h4')):
        vals = re.search(r'constexpr int %s\[\d+\] = \{([^}]*)\}' % name, src).group(1)
        assert [int(v) for v in vals.split(',')] == R.WEIGHTS[s][:2 * s].tolist()
    from tecogan_pytorch_amd import _lib as L
    with pytest.raises(L.TecoganHipError):
        ops.downsample_bi(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), 2)        # CPU tensors are refused
    lib = L.lib()
    assert lib.tg_downsample_bi_u8(None, None, None, 1, 8, 8, 2, 1, None) == -2 and b'null' in lib.tg_last_error_string()
