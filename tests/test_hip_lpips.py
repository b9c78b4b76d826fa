"""GPU: LPIPS (alex / net-lin / v0.1) on the HIP path and reference-style test-mode evaluation.
Kernels against torch-CPU fp64 on the same weights; the metric against the reference's own values
(tests/golden/lpips.npz, make_golden_lpips.py)."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lpips_fixture import CASES, alexnet_state_dict, clip_pair

pytestmark = pytest.mark.gpu

DEV = 'cuda'
EPS32 = 2.0 ** -24


@pytest.fixture(scope='module')
def ops():
    from tecogan_pytorch_amd import ops as o
    return o


def _lin_sd(golden):
    g = golden('lpips')
    return {f'lin{k}.model.1.weight': torch.from_numpy(g[f'lin{k}']) for k in range(5)}


def _make(scaling):
    import tecogan_pytorch_amd  # noqa: F401
    from tecogan_pytorch_amd.metrics.lpips import LPIPS
    g = dict(np.load(os.path.join(os.path.dirname(__file__), 'golden', 'lpips.npz')))
    m = LPIPS(device=DEV, scaling=scaling)
    m.load_alexnet_state_dict(alexnet_state_dict())
    m.load_lin_state_dict({f'lin{k}.model.1.weight': torch.from_numpy(g[f'lin{k}']) for k in range(5)})
    return m


@pytest.fixture(scope='module')
def model():
    """ScalingLayer applied (version '0.1', the string)."""
    return _make(True)


@pytest.fixture(scope='module')
def model_yml():
    """As the reference's ymls run it (version: 0.1, a YAML float): no ScalingLayer."""
    return _make(False)


def _conv_ref(x64, w, b, stride, pad):
    """relu(conv) in fp64 and the error scale sum |x| |w| + |b|."""
    w64, b64 = w.double(), b.double()
    ref = F.relu(F.conv2d(x64, w64, b64, stride=stride, padding=pad))
    mag = F.conv2d(x64.abs(), w64.abs(), b64.abs(), stride=stride, padding=pad)
    return ref, mag


@pytest.mark.parametrize('hw', [(37, 53), (576, 720)])
def test_conv1_uint8_in_matches_fp64(ops, hw):
    from tecogan_pytorch_amd.metrics.lpips import input_lut
    h, w = hw
    sd = alexnet_state_dict()
    wt, b = sd['features.0.weight'], sd['features.0.bias']
    rs = np.random.RandomState(h)
    n0, n1 = (2, 1) if h < 100 else (1, 1)
    x = torch.from_numpy(rs.randint(0, 256, (n0 + n1, h, w, 3)).astype(np.uint8))
    lut = input_lut()
    got = ops.lpips_conv(x[:n0].to(DEV), wt.reshape(64, -1).t().contiguous().to(DEV), b.to(DEV), 64, 11, 4, 2,
                         x1=x[n0:].to(DEV), lut=lut.to(DEV)).cpu().double()
    # the LUT is the reference's fp32 input, exactly: compare with it gathered on the host
    xin = lut[x.long(), torch.arange(3)].permute(0, 3, 1, 2).double()
    ref, mag = _conv_ref(xin, wt, b, 4, 2)
    assert got.shape == ref.shape == (n0 + n1, 64, (h - 7) // 4 + 1, (w - 7) // 4 + 1)
    err = (got - ref).abs()
    tol = 363 * EPS32 * mag + 1e-30
    assert bool((err <= tol).all()), float((err / tol).max())
    assert float((got > 0).double().mean()) > 0.05


@pytest.mark.parametrize('shape', [(3, 64, 23, 31), (1, 64, 71, 89)])
def test_conv5x5_matches_fp64(ops, shape):
    sd = alexnet_state_dict()
    wt, b = sd['features.3.weight'], sd['features.3.bias']
    g = torch.Generator().manual_seed(shape[2])
    x = torch.rand(shape, generator=g) * 2.0
    got = ops.lpips_conv(x.to(DEV), wt.reshape(192, -1).t().contiguous().to(DEV), b.to(DEV), 192, 5, 1, 2).cpu()
    ref, mag = _conv_ref(x.double(), wt, b, 1, 2)
    err = (got.double() - ref).abs()
    tol = 1600 * EPS32 * mag
    assert bool((err <= tol).all()), float((err / tol).max())


@pytest.mark.parametrize('shape', [(2, 5, 15, 15), (1, 64, 143, 179), (3, 7, 8, 10)])
def test_maxpool3s2_is_exact(ops, shape):
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(shape, generator=g)
    got = ops.maxpool3s2(x.to(DEV)).cpu()
    assert torch.equal(got, F.max_pool2d(x, 3, 2))


@pytest.mark.parametrize('variant', ['s', 'ns'])
def test_lpips_matches_reference_fp64(model, model_yml, golden, variant):
    g = golden('lpips')
    m = model if variant == 's' else model_yml
    for name in CASES:
        true, pred = clip_pair(name)
        h, w = min(true.shape[1], pred.shape[1]), min(true.shape[2], pred.shape[2])
        tt = torch.from_numpy(np.ascontiguousarray(true[:, :h, :w])).to(DEV)
        pp = torch.from_numpy(np.ascontiguousarray(pred[:, :h, :w])).to(DEV)
        tot = m(tt, pp).cpu().double().numpy()
        lay = m(tt, pp, per_layer=True).cpu().double().numpy()
        ref64, lay64 = g[f'{name}_{variant}_lpips64'], g[f'{name}_{variant}_layers64']
        bound = 2e-4 * np.abs(ref64) + 1e-9
        lbound = 2e-4 * np.abs(lay64) + 1e-9
        # the bound is the reference's own fp32 accuracy with ~10x room, not fitted to this path
        assert np.all(np.abs(g[f'{name}_{variant}_lpips32'] - ref64) <= bound), name
        assert np.all(np.abs(g[f'{name}_{variant}_layers32'] - lay64) <= lbound), name
        assert np.all(np.abs(tot - ref64) <= bound), (name, tot, ref64)
        assert np.all(np.abs(lay - lay64) <= lbound), (name, lay, lay64)
        # the total is the in-order sum of the layers
        assert np.array_equal(tot.astype(np.float32), (((((lay[:, 0].astype(np.float32) + lay[:, 1].astype(
            np.float32)) + lay[:, 2].astype(np.float32)) + lay[:, 3].astype(np.float32)) + lay[:, 4].astype(
                np.float32))))
    vals = np.concatenate([g[f'{n}_{variant}_lpips64'] for n in CASES])
    assert vals.min() <= 1e-4 and vals.max() >= 1e-2


def test_identity_symmetry_and_determinism(model):
    true, pred = clip_pair('odd100x132_noise2')
    tt, pp = torch.from_numpy(true).to(DEV), torch.from_numpy(pred).to(DEV)
    assert torch.equal(model(tt, tt).cpu(), torch.zeros(3))
    ab, ba = model(tt, pp).cpu(), model(pp, tt).cpu()
    assert torch.allclose(ab, ba, rtol=1e-6, atol=0)
    r1 = model(tt, pp, per_layer=True).cpu()
    r2 = model(tt, pp, per_layer=True).cpu()
    assert torch.equal(r1, r2)
    old = model.chunk_frames
    try:
        for chunk in (1, 2):
            model.chunk_frames = chunk
            assert torch.equal(model(tt, pp, per_layer=True).cpu(), r1), chunk
        model.chunk_frames = None
        perm = torch.tensor([2, 0, 1])
        rp = model(tt[perm.to(DEV)].contiguous(), pp[perm.to(DEV)].contiguous(), per_layer=True).cpu()
        assert torch.equal(rp, r1[perm])
        # a frame evaluated with different neighbours in the batch
        t2 = torch.cat([tt[1:2], tt[1:2], tt[0:1]]).contiguous()
        p2 = torch.cat([pp[1:2], tt[1:2], pp[0:1]]).contiguous()
        r3 = model(t2, p2, per_layer=True).cpu()
        assert torch.equal(r3[0], r1[1]) and torch.equal(r3[2], r1[0]) and float(r3[1].abs().sum()) == 0.0
    finally:
        model.chunk_frames = old
    with pytest.raises(ValueError):
        model(tt[:, :30].contiguous(), pp[:, :30].contiguous())


def _metric_opt():
    return {'device': 'cuda', 'dist': False, 'rank': 0,
            'metric': {'PSNR': {'colorspace': 'y'},
                       'LPIPS': {'model': 'net-lin', 'net': 'alex', 'colorspace': 'rgb', 'spatial': False,
                                 'version': 0.1},
                       'tOF': {'colorspace': 'y'}}}


def test_metric_calculator_matches_reference(model_yml, golden):
    """The reference's MetricCalculator as its ymls configure it (version: 0.1 -> no ScalingLayer)."""
    from tecogan_pytorch_amd.metrics.metric_calculator import MetricCalculator
    g = golden('lpips')
    mc = MetricCalculator(_metric_opt(), lpips=model_yml)
    names = ['crop130x170_noise40', 'min64_noise1', 'vid4_576x720_noise40']
    for i, name in enumerate(names):
        true, pred = clip_pair(name)
        if i == 0:                                       # numpy in (uploaded), cropped to the smaller frame
            mc.compute_sequence_metrics(name, true, pred)
        else:
            mc.compute_sequence_metrics(name, torch.from_numpy(true).to(DEV), torch.from_numpy(pred).to(DEV))
        md = mc.metric_dict[name]
        assert list(md) == ['PSNR', 'LPIPS']
        assert np.all(np.abs(np.array(md['PSNR']) - g[f'{name}_psnr']) <= 1e-3), name
        ref64 = g[f'{name}_ns_lpips64']
        assert np.all(np.abs(g[f'{name}_mc32'] - ref64) <= 2e-4 * np.abs(ref64) + 1e-9), name
        assert np.all(np.abs(np.array(md['LPIPS']) - ref64) <= 2e-4 * np.abs(ref64) + 1e-9), name
    mc.gather(names)
    avg = mc.average()
    exp = np.mean([np.mean(g[f'{n}_ns_lpips64']) for n in names])
    assert abs(avg['LPIPS'] - exp) <= 2e-4 * exp
    assert abs(avg['PSNR'] - np.mean([np.mean(g[f'{n}_psnr']) for n in names])) <= 1e-3


def test_main_test_mode_on_png_folders(tmp_path, model_yml, golden):
    import yaml
    from PIL import Image
    from procedural_weights import generator_state_dict, smooth_clip
    from tecogan_pytorch_amd import main as M
    from tecogan_pytorch_amd.metrics.psnr import compute_psnr
    from tecogan_pytorch_amd.models import define_model
    torch.save(generator_state_dict(scale=4, degradation='BD'), str(tmp_path / 'G_iter30.pth'))
    torch.save(alexnet_state_dict(), str(tmp_path / 'alexnet.pth'))
    torch.save(_lin_sd(golden), str(tmp_path / 'alex.pth'))
    seqs = {}
    for i, key in enumerate(['calendar', 'city']):
        gt = (smooth_clip(3, 3, 128, 160, seed=40 + i).permute(0, 2, 3, 1) * 255).round().clamp(0, 255)
        gt = gt.to(torch.uint8).numpy()
        seqs[key] = gt
        for f in range(3):
            p = tmp_path / 'GT' / key / f'{f:08d}.png'
            p.parent.mkdir(parents=True, exist_ok=True)
            Image.fromarray(gt[f]).save(str(p))
    opt = M.default_opt()
    opt['model']['name'] = 'FRVSR'
    opt['model']['generator']['load_path'] = str(tmp_path / 'G_iter30.pth')
    opt['dataset']['test'] = {'name': 'Vid4', 'gt_seq_dir': str(tmp_path / 'GT'), 'lr_seq_dir': None}
    opt['test'].update({'save_res': True, 'res_dir': str(tmp_path / 'res'), 'save_json': True,
                        'json_dir': str(tmp_path / 'json'), 'num_pad_front': 2})
    opt['metric'] = _metric_opt()['metric']
    opt['metric']['LPIPS'].update(net_path=str(tmp_path / 'alexnet.pth'), lin_path=str(tmp_path / 'alex.pth'))
    (tmp_path / 'test.yml').write_text(yaml.safe_dump(opt, sort_keys=False))
    M.main(['--mode', 'test', '--exp_dir', str(tmp_path), '--opt', 'test.yml'])
    got = json.load(open(tmp_path / 'json' / 'Vid4_avg.json'))
    assert list(got) == ['G_iter30'] and list(got['G_iter30']) == ['PSNR', 'LPIPS']
    # expected: the reference protocol on the host frames (compute_PSNR), LPIPS of the saved results
    o = dict(opt, dist=False, device='cuda', rank=0, world_size=1, is_train=False)
    m = define_model(o)
    psnr, lp = [], []
    for key, gt in seqs.items():
        m.prepare_inference_data({'gt': torch.from_numpy(gt)})
        hr = m.infer()
        saved = np.stack([np.asarray(Image.open(tmp_path / 'res' / 'Vid4' / 'G_iter30' / key / f'{f:08d}.png'))
                          for f in range(3)])
        assert np.array_equal(saved, hr)
        psnr.append(np.mean([compute_psnr(gt[f], hr[f]) for f in range(3)]))
        lp.append(float(model_yml(torch.from_numpy(gt).to(DEV), torch.from_numpy(hr).to(DEV)).double().mean()))
    assert abs(float(got['G_iter30']['PSNR']) - np.mean(psnr)) <= 2e-6 + 1e-3
    assert abs(float(got['G_iter30']['LPIPS']) - np.mean(lp)) <= 1e-6
    assert 0.0 < np.mean(lp) and 5.0 < np.mean(psnr) < 60.0
