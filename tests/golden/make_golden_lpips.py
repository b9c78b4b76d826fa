#!/usr/bin/env python
"""Golden vectors of the LPIPS metric, produced by the upstream reference on CPU (authoring
container only; the make_golden_feat.py pattern).

The reference's LPIPS builds `torchvision.models.alexnet(pretrained=True).features`; torchvision is
not installed, so the import stub's `torchvision.models.alexnet` returns the features[0:12] layer
stack carrying the PROCEDURAL weights of lpips_fixture.alexnet_state_dict.  The lin weights are the
reference's own `weights/v0.1/alex.pth`.  Everything else -- MetricCalculator (PSNR-y + LPIPS), the
[-1, 1] scaling, ScalingLayer, normalize_tensor, the lin layers, the spatial mean, the crop of
differently sized frames -- is the reference's code, run in fp32 and (PNetLin only) in fp64, with
and without ScalingLayer (see the note in main()).

Output: tests/golden/lpips.npz"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _ref_import  # noqa: E402
from lpips_fixture import CASES, alexnet_state_dict, clip_pair, crc  # noqa: E402

LIN_PATH = os.path.join(_ref_import.REF_CODES, 'metrics', 'LPIPS', 'models', 'weights', 'v0.1', 'alex.pth')


class _AlexNet(nn.Module):
    def __init__(self):
        super().__init__()
        self.features = nn.Sequential(
            nn.Conv2d(3, 64, 11, 4, 2), nn.ReLU(inplace=True), nn.MaxPool2d(3, 2),
            nn.Conv2d(64, 192, 5, padding=2), nn.ReLU(inplace=True), nn.MaxPool2d(3, 2),
            nn.Conv2d(192, 384, 3, padding=1), nn.ReLU(inplace=True),
            nn.Conv2d(384, 256, 3, padding=1), nn.ReLU(inplace=True),
            nn.Conv2d(256, 256, 3, padding=1), nn.ReLU(inplace=True),
            nn.MaxPool2d(3, 2))
        self.load_state_dict(alexnet_state_dict(), strict=True)


def main():
    _ref_import.import_reference()
    sys.modules['torchvision.models'].alexnet = lambda pretrained=True: _AlexNet()
    import logging
    logging.getLogger('base').setLevel(logging.ERROR)
    from metrics.metric_calculator import MetricCalculator
    torch.set_num_threads(8)
    opt = {'device': 'cpu', 'dist': False, 'rank': 0,
           'metric': {'PSNR': {'colorspace': 'y'},
                      'LPIPS': {'model': 'net-lin', 'net': 'alex', 'colorspace': 'rgb', 'spatial': False,
                                'version': 0.1}}}
    mc = MetricCalculator(opt)
    assert not mc.dm.net.training
    import copy
    import metrics.LPIPS.models as util
    from metrics.LPIPS.models.networks_basic import spatial_average
    lin_sd = torch.load(LIN_PATH, map_location='cpu')
    d = {f'lin{k}': lin_sd[f'lin{k}.model.1.weight'].numpy().astype(np.float32) for k in range(5)}
    # PNetLin applies ScalingLayer only when version == '0.1' (a string).  The reference's ymls write
    # `version: 0.1`, which YAML reads as a float, so MetricCalculator runs WITHOUT it; DistModel's own
    # default (the string) runs with it.  Both variants are recorded: 's' (scaled) and 'ns'.
    nets = {}
    for v, version in (('s', '0.1'), ('ns', 0.1)):
        n32 = copy.deepcopy(mc.dm.net).eval()
        n32.version = version
        nets[v] = (n32, copy.deepcopy(n32).double())
    for k in range(5):
        assert np.array_equal(d[f'lin{k}'], getattr(nets['s'][0], f'lin{k}').model[1].weight.detach().numpy())

    def per_layer(net, a, b):
        """PNetLin.forward(retPerLayer=True) returns res[0] after `val += res[l]` (the same tensor):
        layer 0 is recomputed with the reference's own pieces."""
        val, res = net(a, b, retPerLayer=True)
        res = [r.item() for r in res]
        i0, i1 = (net.scaling_layer(a), net.scaling_layer(b)) if net.version == '0.1' else (a, b)
        o0, o1 = net.net.forward(i0)[0], net.net.forward(i1)[0]
        diff = (util.normalize_tensor(o0) - util.normalize_tensor(o1)) ** 2
        res[0] = spatial_average(net.lins[0].model(diff), keepdim=True).item()
        return val.item(), res

    d['cases'] = np.array(list(CASES))
    for name in CASES:
        true, pred = clip_pair(name)
        d[f'{name}_crc'] = np.array([crc(true), crc(pred)], dtype=np.uint64)
        d[f'{name}_shape'] = np.array([true.shape, pred.shape])
        mc.reset()
        mc.compute_sequence_metrics(name, true, pred)
        d[f'{name}_psnr'] = np.array(mc.metric_dict[name]['PSNR'], dtype=np.float64)
        d[f'{name}_mc32'] = np.array(mc.metric_dict[name]['LPIPS'], dtype=np.float64)
        h, w = min(true.shape[1], pred.shape[1]), min(true.shape[2], pred.shape[2])
        for v, (n32, n64) in nets.items():
            rows = {'t32': [], 'l32': [], 't64': [], 'l64': []}
            for i in range(true.shape[0]):
                a = torch.FloatTensor(np.ascontiguousarray(true[i, :h, :w])).unsqueeze(0).permute(0, 3, 1, 2)
                b = torch.FloatTensor(np.ascontiguousarray(pred[i, :h, :w])).unsqueeze(0).permute(0, 3, 1, 2)
                a, b = a * 2.0 / 255.0 - 1.0, b * 2.0 / 255.0 - 1.0
                with torch.no_grad():
                    t32, l32 = per_layer(n32, a, b)
                    t64, l64 = per_layer(n64, a.double(), b.double())
                for key, val in (('t32', t32), ('l32', l32), ('t64', t64), ('l64', l64)):
                    rows[key].append(val)
            d[f'{name}_{v}_lpips32'] = np.array(rows['t32'])
            d[f'{name}_{v}_layers32'] = np.array(rows['l32'])
            d[f'{name}_{v}_lpips64'] = np.array(rows['t64'])
            d[f'{name}_{v}_layers64'] = np.array(rows['l64'])
            err = np.max(np.abs(d[f'{name}_{v}_lpips32'] - d[f'{name}_{v}_lpips64']) / d[f'{name}_{v}_lpips64'])
            print(f'{name} [{v}]: lpips64 {rows["t64"]}  fp32 max rel err {err:.2e}')
        assert np.array_equal(d[f'{name}_mc32'], d[f'{name}_ns_lpips32'])
        print(f'    psnr {d[f"{name}_psnr"].round(3)}')
    path = os.path.join(HERE, 'lpips.npz')
    np.savez_compressed(path, **d)
    print('lpips.npz', os.path.getsize(path) // 1024, 'KiB')


if __name__ == '__main__':
    main()
