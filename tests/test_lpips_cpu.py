"""CPU side of the LPIPS / MetricCalculator feature: fixture inputs, weight loaders, metric-section
validation, the PNG-folder reader, the JSON format of MetricCalculator.save and the cross-rank
gather (gloo, world size 2).  No kernel is launched here."""
import json
import logging
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from lpips_fixture import CASES, alexnet_state_dict, clip_pair, crc


def _lin_sd(golden):
    g = golden('lpips')
    return {f'lin{k}.model.1.weight': torch.from_numpy(g[f'lin{k}']) for k in range(5)}


def _lpips_cpu(golden):
    from tecogan_pytorch_amd.metrics.lpips import LPIPS
    m = LPIPS(device='cpu')
    m.load_alexnet_state_dict(alexnet_state_dict())
    m.load_lin_state_dict(_lin_sd(golden))
    return m


def test_fixture_inputs_match_golden_crc(golden):
    g = golden('lpips')
    assert list(g['cases']) == list(CASES)
    for name in CASES:
        true, pred = clip_pair(name)
        assert [crc(true), crc(pred)] == [int(v) for v in g[f'{name}_crc']], name
        assert np.array_equal(np.array([true.shape, pred.shape]), g[f'{name}_shape'])


def test_weight_loaders_accept_reference_formats_and_reject_bad_ones(golden):
    from tecogan_pytorch_amd.metrics.lpips import LPIPS
    sd = alexnet_state_dict()
    tv = dict(sd)
    tv['classifier.1.weight'] = torch.zeros(4096, 9216)          # torchvision's classifier keys are ignored
    tv['classifier.1.bias'] = torch.zeros(4096)
    m = LPIPS(device='cpu')
    m.load_alexnet_state_dict(tv)
    m.load_lin_state_dict(_lin_sd(golden))
    own = m.state_dict()
    assert all(torch.equal(own[k], sd[k]) for k in sd)
    assert sorted(k for k in own if k.startswith('lin')) == [f'lin{k}.model.1.weight' for k in range(5)]
    m2 = LPIPS(device='cpu')
    m2.load_alexnet_state_dict(own)                                # the module's own state dict
    m2.load_lin_state_dict(own)
    assert all(torch.equal(m2.state_dict()[k], v) for k, v in own.items())
    bad = dict(sd)
    del bad['features.8.bias']
    with pytest.raises(KeyError, match='features.8.bias'):
        LPIPS(device='cpu').load_alexnet_state_dict(bad)
    bad = dict(sd)
    bad['features.3.weight'] = torch.zeros(192, 64, 3, 3)
    with pytest.raises(ValueError, match='features.3'):
        LPIPS(device='cpu').load_alexnet_state_dict(bad)
    lin = _lin_sd(golden)
    del lin['lin4.model.1.weight']
    with pytest.raises(KeyError, match='lin4'):
        LPIPS(device='cpu').load_lin_state_dict(lin)
    lin = _lin_sd(golden)
    lin['lin2.model.1.weight'] = torch.zeros(1, 256, 1, 1)
    with pytest.raises(ValueError, match='lin2'):
        LPIPS(device='cpu').load_lin_state_dict(lin)


def test_missing_weight_files_name_both_ways_to_supply_them(tmp_path, monkeypatch, golden):
    from tecogan_pytorch_amd.metrics.lpips import LPIPS
    monkeypatch.setenv('TORCH_HOME', str(tmp_path))
    monkeypatch.delenv('TECOGAN_ALEXNET_PTH', raising=False)
    monkeypatch.delenv('TECOGAN_LPIPS_LIN_PTH', raising=False)
    with pytest.raises(FileNotFoundError) as e:
        LPIPS.from_config({}, device='cpu')
    assert 'net_path' in str(e.value) and 'TECOGAN_ALEXNET_PTH' in str(e.value)
    assert str(tmp_path / 'hub' / 'checkpoints' / 'alexnet-owt-7be5be79.pth') in str(e.value)
    net = tmp_path / 'hub' / 'checkpoints' / 'alexnet-owt-7be5be79.pth'
    net.parent.mkdir(parents=True)
    torch.save(alexnet_state_dict(), str(net))                    # found at torchvision's cache path
    with pytest.raises(FileNotFoundError) as e:
        LPIPS.from_config({}, device='cpu')
    assert 'lin_path' in str(e.value) and 'TECOGAN_LPIPS_LIN_PTH' in str(e.value)
    lin = tmp_path / 'alex.pth'
    torch.save(_lin_sd(golden), str(lin))
    monkeypatch.setenv('TECOGAN_LPIPS_LIN_PTH', str(lin))
    m = LPIPS.from_config({}, device='cpu')
    assert torch.equal(m.state_dict()['lin0.model.1.weight'], _lin_sd(golden)['lin0.model.1.weight'])


def test_scaling_layer_follows_the_version_type_as_in_the_reference(tmp_path, golden):
    """PNetLin compares `version == '0.1'`: the ymls' float 0.1 skips ScalingLayer, the string applies it."""
    from tecogan_pytorch_amd.metrics.lpips import LPIPS, applies_scaling, input_lut
    assert applies_scaling('0.1') and applies_scaling(None) and not applies_scaling(0.1)
    assert torch.equal(input_lut(False)[:, 0], torch.arange(256, dtype=torch.float32) * 2.0 / 255.0 - 1.0)
    assert torch.equal(input_lut(True)[255], (torch.ones(3) - torch.tensor([-.030, -.088, -.188]))
                       / torch.tensor([.458, .448, .450]))
    torch.save(alexnet_state_dict(), str(tmp_path / 'a.pth'))
    torch.save(_lin_sd(golden), str(tmp_path / 'l.pth'))
    paths = {'net_path': str(tmp_path / 'a.pth'), 'lin_path': str(tmp_path / 'l.pth')}
    assert not LPIPS.from_config(dict(paths, version=0.1), device='cpu').scaling
    assert LPIPS.from_config(dict(paths, version='0.1'), device='cpu').scaling


def test_metric_section_validation(golden, caplog):
    from tecogan_pytorch_amd.metrics.metric_calculator import MetricCalculator
    lp = _lpips_cpu(golden)
    base = {'device': 'cpu', 'dist': False, 'rank': 0}
    lcfg = {'model': 'net-lin', 'net': 'alex', 'colorspace': 'rgb', 'spatial': False, 'version': 0.1}
    with caplog.at_level(logging.WARNING):
        mc = MetricCalculator(dict(base, metric={'PSNR': {'colorspace': 'y'}, 'LPIPS': lcfg,
                                                 'tOF': {'colorspace': 'y'}}), lpips=lp)
    assert list(mc.metric_opt) == ['PSNR', 'LPIPS']
    assert sum('tOF' in r.getMessage() for r in caplog.records) == 1
    for key, val in (('spatial', True), ('net', 'vgg'), ('model', 'net'), ('version', 0.0)):
        with pytest.raises(ValueError, match=key):
            MetricCalculator(dict(base, metric={'LPIPS': dict(lcfg, **{key: val})}), lpips=lp)
    with pytest.raises(ValueError):
        MetricCalculator(dict(base, metric={'SSIM': {}}))


def test_png_folder_reader(tmp_path):
    from PIL import Image
    from tecogan_pytorch_amd.data.folder_dataset import FolderDataset, retrieve_files
    rs = np.random.RandomState(0)
    frames = {}
    for root, hw in (('gt', (12, 16)), ('lr', (3, 4))):
        for key in ('000', '011', '015', '020'):
            for rel in ('b/0001.png', 'a/0003.png', '0002.png', 'a/0000.jpg'):
                p = tmp_path / root / key / rel
                p.parent.mkdir(parents=True, exist_ok=True)
                img = rs.randint(0, 256, (hw[0], hw[1], 3)).astype(np.uint8)
                Image.fromarray(img).save(str(p), format='PNG')     # lossless even under a .jpg name
                frames[(root, key, rel)] = img
            (tmp_path / root / key / 'notes.txt').write_text('not a frame')
    (tmp_path / 'gt' / '099').mkdir()                               # only in gt: not paired
    files = retrieve_files(str(tmp_path / 'gt' / '011'))
    order = ['0002.png', 'a/0000.jpg', 'a/0003.png', 'b/0001.png']  # recursive, sorted by path, png|jpg only
    assert files == [str(tmp_path / 'gt' / '011' / r) for r in order]
    ds = FolderDataset({'gt_seq_dir': str(tmp_path / 'gt'), 'lr_seq_dir': str(tmp_path / 'lr'),
                        'filter_list': ['020', '011', '999']})
    assert ds.keys == ['011', '020']
    d = ds[1]
    assert d['seq_idx'] == '020' and d['gt'].dtype == torch.uint8 and d['lr'].dtype == torch.float32
    assert tuple(d['gt'].shape) == (4, 12, 16, 3) and tuple(d['lr'].shape) == (4, 3, 4, 3)
    for i, rel in enumerate(order):
        assert np.array_equal(d['gt'][i].numpy(), frames[('gt', '020', rel)])
        assert np.array_equal(d['lr'][i].numpy(), frames[('lr', '020', rel)].astype(np.float32) / 255.0)
    assert FolderDataset({'gt_seq_dir': str(tmp_path / 'gt')}).keys == ['000', '011', '015', '020', '099']
    ff = tmp_path / 'keys.txt'
    ff.write_text('015\n000\n')
    assert FolderDataset({'gt_seq_dir': str(tmp_path / 'gt'), 'filter_file': str(ff)}).keys == ['000', '015']
    with pytest.raises(ValueError):
        FolderDataset({'gt_seq_dir': str(tmp_path / 'gt')}, degradation='BI')


def test_save_writes_the_reference_json_format(tmp_path):
    from collections import OrderedDict
    from tecogan_pytorch_amd.metrics.metric_calculator import MetricCalculator
    mc = MetricCalculator({'device': 'cpu', 'dist': False, 'rank': 0, 'metric': {'PSNR': {'colorspace': 'y'}}})
    mc.avg_metric_dict = OrderedDict([('a', {'PSNR': 30.0}), ('b', {'PSNR': 31.5})])
    path = str(tmp_path / 'Vid4_avg.json')
    mc.save('G_iter500', path)
    mc.avg_metric_dict = OrderedDict([('a', {'PSNR': 20.0})])
    mc.save('G_iter40', path)
    mc.save('G_iter500', path)                       # existing entries are kept unless override
    with open(path) as f:
        text = f.read()
    assert text == ('{\n    "G_iter40": {\n        "PSNR": "20.000000"\n    },\n'
                    '    "G_iter500": {\n        "PSNR": "30.750000"\n    }\n}')
    mc.save('G_iter500', path, override=True)
    assert json.load(open(path))['G_iter500'] == {'PSNR': '20.000000'}


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _gather_worker(rank, world, port, out):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    from tecogan_pytorch_amd.utils import dist_utils as D
    from tecogan_pytorch_amd.metrics.metric_calculator import MetricCalculator
    opt = {}
    D.init_dist(opt, rank, backend='gloo')
    opt.update(device='cpu', metric={'PSNR': {'colorspace': 'y'}})
    mc = MetricCalculator(opt)
    seqs = ['s0', 's1', 's2']
    for i in D.shard_indices(len(seqs)):            # per-frame lists on the rank that owns the sequence
        mc.metric_dict[seqs[i]] = {'PSNR': [10.0 * (i + 1), 10.0 * (i + 1) + 2.0 * (rank + 1)]}
    mc.gather(seqs)
    out[rank] = (dict((k, dict(v)) for k, v in mc.avg_metric_dict.items()),
                 dict(mc.average()) if rank == 0 else None)
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_gather_sums_sequence_means_over_ranks_to_master():
    port = _free_port()
    mgr = mp.Manager()
    try:
        out = mgr.dict()
        mp.spawn(_gather_worker, args=(2, port, out), nprocs=2, join=True)
        a, b = out[0], out[1]
    finally:
        mgr.shutdown()                               # no helper process outlives the test
    # s0, s2 on rank 0 (mean 10 + 1, 30 + 1), s1 on rank 1 (mean 20 + 2)
    assert a[0] == {'s0': {'PSNR': 11.0}, 's1': {'PSNR': 22.0}, 's2': {'PSNR': 31.0}}
    assert list(a[0]) == ['s0', 's1', 's2']
    assert b[0] == {}                                # only rank 0 holds the results
    assert a[1] == {'PSNR': pytest.approx(64.0 / 3)}
