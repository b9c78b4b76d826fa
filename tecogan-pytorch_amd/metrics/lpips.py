"""LPIPS v0.1 with net='alex', model='net-lin', spatial=False on the HIP path
(codes/metrics/LPIPS/models/networks_basic.py:25-99, pretrained_networks.py:57-95,
metric_calculator.py:246-261).

Backbone: torchvision alexnet().features[0:12], taps relu1..relu5.  The reference builds it with
`tv.alexnet(pretrained=True)`; there is no torchvision (and no network) here, so the architecture
is restated and the weights come from files the user supplies, as for the perceptual-loss VGG19
(models/networks/vgg_nets.py):
  * AlexNet: a torchvision `alexnet` state dict (`features.{0,3,6,8,10}.*`, classifier keys ignored)
    or this module's own; default `$TORCH_HOME/hub/checkpoints/alexnet-owt-7be5be79.pth`, where a
    reference user's torchvision has already cached it.
  * lin layers: the reference's `weights/v0.1/alex.pth` (`lin{k}.model.1.weight`, (1, C, 1, 1)).

ScalingLayer runs only when the metric section's `version` is the string '0.1' (applies_scaling):
the reference's ymls say `version: 0.1`, a YAML float, and PNetLin compares with the string, so the
reference's own TecoGAN evaluations skip it.  Both forms are supported and tested.

Kernels: conv1 reads the uint8 HWC frames directly (the [-1, 1] scaling and ScalingLayer are a
256 x 3 table built here with the reference's op order, so the fp32 input is bit-exact), conv2 is
the same implicit-GEMM kernel at k5 / s1, conv3..5 the conv3x3 kernel with fused ReLU, the pools
tg_maxpool3s2_fwd, the head tg_lpips_head (deterministic)."""
import os

import torch

from .. import ops
from .._lib import ACT_RELU, TecoganHipError

# (features index, cin, cout, kernel, stride, padding); a MaxPool2d(3, 2) follows conv 0 and conv 1
ALEX_CONVS = [(0, 3, 64, 11, 4, 2), (3, 64, 192, 5, 1, 2), (6, 192, 384, 3, 1, 1),
              (8, 384, 256, 3, 1, 1), (10, 256, 256, 3, 1, 1)]
CHNS = [64, 192, 384, 256, 256]
SHIFT = [-.030, -.088, -.188]
SCALE = [.458, .448, .450]
_MIN_HW = 31             # conv1 must give >= 7 rows / columns so that both pools give >= 1


def default_alexnet_path():
    home = os.environ.get('TORCH_HOME') or os.path.join(
        os.environ.get('XDG_CACHE_HOME') or os.path.join(os.path.expanduser('~'), '.cache'), 'torch')
    return os.path.join(home, 'hub', 'checkpoints', 'alexnet-owt-7be5be79.pth')


def applies_scaling(version):
    """PNetLin runs ScalingLayer only when `version == '0.1'` -- the string (networks_basic.py:66).
    The reference's ymls write `version: 0.1`, which YAML reads as a float: their LPIPS numbers are
    computed WITHOUT ScalingLayer.  A quoted '0.1' (or no version: DistModel's default) applies it."""
    return version is None or version == '0.1'


def input_lut(scaling=True):
    """(256, 3) fp32: byte v of channel c -> v * 2.0 / 255.0 - 1.0 (metric_calculator.py:250-256), then
    ScalingLayer when `scaling` (networks_basic.py:94-101); the reference's fp32 ops in its order."""
    v = torch.arange(256, dtype=torch.float32).view(256, 1).expand(256, 3)
    x = v * 2.0 / 255.0 - 1.0
    if not scaling:
        return x.contiguous()
    shift = torch.tensor(SHIFT, dtype=torch.float32).view(1, 3)
    scale = torch.tensor(SCALE, dtype=torch.float32).view(1, 3)
    return ((x - shift) / scale).contiguous()


def alexnet_out_sizes(h, w):
    """[(h, w)] of relu1..relu5."""
    if h < _MIN_HW or w < _MIN_HW:
        raise ValueError(f'LPIPS (alex) needs frames of at least {_MIN_HW} x {_MIN_HW}, got {h} x {w}')
    h1, w1 = (h + 4 - 11) // 4 + 1, (w + 4 - 11) // 4 + 1
    p1 = ((h1 - 3) // 2 + 1, (w1 - 3) // 2 + 1)
    p2 = ((p1[0] - 3) // 2 + 1, (p1[1] - 3) // 2 + 1)
    return [(h1, w1), p1, p2, p2, p2]


def image_bytes(h, w):
    """Device bytes one image of the backbone holds (taps + pool outputs)."""
    s = alexnet_out_sizes(h, w)
    floats = sum(c * a * b for c, (a, b) in zip(CHNS, s)) + 64 * s[1][0] * s[1][1] + 192 * s[2][0] * s[2][1]
    return 4 * floats


class LPIPS:
    """LPIPS(alex, net-lin, v0.1) of uint8 frames on the device.  Weights: load_alexnet_state_dict and
    load_lin_state_dict (or from_config).  scaling: whether ScalingLayer runs (applies_scaling).
    chunk_frames bounds memory (None: a budget of mem_budget bytes); results do not depend on it."""

    def __init__(self, device='cuda', chunk_frames=None, mem_budget=2 << 30, scaling=True):
        self.device = torch.device(device)
        self.scaling = bool(scaling)
        self.chunk_frames = chunk_frames
        self.mem_budget = mem_budget
        self.alex = None          # [(weight, bias)] of features.{0,3,6,8,10}, fp32 on the host
        self.lin = None           # [(C_k,)] fp32 on the host
        self._packed = None

    # ---- weights -------------------------------------------------------------------------------
    def load_alexnet_state_dict(self, sd):
        """torchvision alexnet state dict (`features.{0,3,6,8,10}.weight/bias`; classifier keys are
        ignored) or this module's own (the same keys)."""
        conv = []
        for idx, ci, co, k, _, _ in ALEX_CONVS:
            kw, kb = f'features.{idx}.weight', f'features.{idx}.bias'
            if kw not in sd or kb not in sd:
                raise KeyError(f'AlexNet weights: missing {kw if kw not in sd else kb}')
            w, b = sd[kw], sd[kb]
            if tuple(w.shape) != (co, ci, k, k) or tuple(b.shape) != (co,):
                raise ValueError(f'AlexNet weights: features.{idx} has shapes {tuple(w.shape)} / {tuple(b.shape)}, '
                                 f'expected {(co, ci, k, k)} / {(co,)}')
            conv.append((w.detach().to(torch.float32).cpu(), b.detach().to(torch.float32).cpu()))
        self.alex = conv
        self._packed = None

    def _device_weights(self):
        """Upload / pack the AlexNet weights on first use (the loaders work without a device)."""
        if self._packed is None:
            if self.alex is None or self.lin is None:
                raise RuntimeError('LPIPS: weights not loaded (load_alexnet_state_dict / load_lin_state_dict)')
            packed = []
            for (idx, ci, co, k, _, _), (w, b) in zip(ALEX_CONVS, self.alex):
                dw, db = w.to(self.device).contiguous(), b.to(self.device).contiguous()
                if k == 3:
                    wpk, _, _, ocb = ops.pack_conv3x3(dw)
                    packed.append((wpk, db, ocb, ci, co))
                else:                     # (K, cout) for the implicit-GEMM kernel: a layout change at load
                    packed.append((w.reshape(co, -1).t().contiguous().to(self.device), db, None, ci, co))
            self._packed = (packed, [v.to(self.device).contiguous() for v in self.lin],
                            input_lut(self.scaling).to(self.device))
        return self._packed

    def load_lin_state_dict(self, sd):
        """The reference's lin weights: `lin{k}.model.1.weight`, shape (1, C_k, 1, 1)."""
        lin = []
        for k, c in enumerate(CHNS):
            key = f'lin{k}.model.1.weight'
            if key not in sd:
                raise KeyError(f'LPIPS lin weights: missing {key}')
            v = sd[key]
            if tuple(v.shape) != (1, c, 1, 1):
                raise ValueError(f'LPIPS lin weights: {key} has shape {tuple(v.shape)}, expected {(1, c, 1, 1)}')
            lin.append(v.detach().to(torch.float32).cpu().reshape(c).contiguous())
        self.lin = lin
        self._packed = None

    def state_dict(self):
        if self.alex is None or self.lin is None:
            raise RuntimeError('LPIPS: weights not loaded')
        sd = {}
        for (idx, *_), (w, b) in zip(ALEX_CONVS, self.alex):
            sd[f'features.{idx}.weight'], sd[f'features.{idx}.bias'] = w.clone(), b.clone()
        for k, v in enumerate(self.lin):
            sd[f'lin{k}.model.1.weight'] = v.clone().view(1, -1, 1, 1)
        return sd

    @classmethod
    def from_config(cls, cfg, device='cuda', **kw):
        """Metric section `LPIPS:` of the yml: net_path / lin_path, else $TECOGAN_ALEXNET_PTH /
        $TECOGAN_LPIPS_LIN_PTH; net_path defaults to torchvision's cache file.  ScalingLayer follows
        the section's `version` as in the reference (applies_scaling)."""
        cfg = cfg or {}
        kw.setdefault('scaling', applies_scaling(cfg.get('version')))
        net_path = cfg.get('net_path') or os.environ.get('TECOGAN_ALEXNET_PTH') or default_alexnet_path()
        lin_path = cfg.get('lin_path') or os.environ.get('TECOGAN_LPIPS_LIN_PTH')
        if not os.path.isfile(net_path):
            raise FileNotFoundError(
                f'LPIPS needs the ImageNet AlexNet weights: {net_path} does not exist.  Set metric.LPIPS.net_path '
                '(or TECOGAN_ALEXNET_PTH) to a torchvision alexnet state dict (alexnet-owt-7be5be79.pth)')
        if not lin_path or not os.path.isfile(lin_path):
            raise FileNotFoundError(
                f'LPIPS needs the v0.1 alex linear-layer weights ({lin_path or "no path given"}).  Set '
                'metric.LPIPS.lin_path (or TECOGAN_LPIPS_LIN_PTH) to the reference\'s '
                'codes/metrics/LPIPS/models/weights/v0.1/alex.pth')
        m = cls(device=device, **kw)
        m.load_alexnet_state_dict(torch.load(net_path, map_location='cpu'))
        m.load_lin_state_dict(torch.load(lin_path, map_location='cpu'))
        return m

    # ---- forward -------------------------------------------------------------------------------
    def _chunk(self, t, h, w):
        if self.chunk_frames:
            return max(1, int(self.chunk_frames))
        return max(1, min(t, int(self.mem_budget // (2 * image_bytes(h, w)))))

    def features(self, x0, x1=None):
        """relu1..relu5 of the uint8 frames x0 (then x1) as one batch: list of (n,c,h,w) fp32."""
        packed, _, lut = self._device_weights()
        feats = []
        wt, b, _, _, co = packed[0]
        y = ops.lpips_conv(x0, wt, b, co, 11, 4, 2, x1=x1, lut=lut)
        feats.append(y)
        y = ops.maxpool3s2(y)
        wt, b, _, _, co = packed[1]
        y = ops.lpips_conv(y, wt, b, co, 5, 1, 2)
        feats.append(y)
        y = ops.maxpool3s2(y)
        for wpk, b, ocb, cin, cout in packed[2:]:
            out = torch.empty(y.shape[0], cout, y.shape[2], y.shape[3], dtype=torch.float32, device=y.device)
            # one image per launch: the conv3x3 kernel picks its variant (and K order) from the batch
            # size, and a frame's value must not depend on the batch it was evaluated in
            for i in range(y.shape[0]):
                ops.conv3x3(y[i:i + 1], wpk, b, cin, cout, ocb, act=ACT_RELU, out=out[i:i + 1], ksplit=1)
            feats.append(out)
            y = out
        return feats

    def features_of(self, seq_u8):
        """relu1..relu5 of every frame of a (t,h,w,3) uint8 device clip: list of five (t,c,h,w) fp32 tensors,
        computed in chunks of _chunk frames.  A frame's taps do not depend on the chunking or on the other
        frames (see features), so distance() on them gives forward()'s values bit for bit; a metric that needs
        one frame in several pairs (tLP) runs the backbone once per frame."""
        self._device_weights()
        if not (torch.is_tensor(seq_u8) and seq_u8.is_cuda and seq_u8.dtype == torch.uint8 and seq_u8.dim() == 4
                and seq_u8.shape[3] == 3):
            raise TecoganHipError(f'LPIPS: frames must be a (t,h,w,3) uint8 device tensor, got '
                                  f'{getattr(seq_u8, "dtype", type(seq_u8))} {tuple(getattr(seq_u8, "shape", ()))}')
        t, h, w, _ = seq_u8.shape
        alexnet_out_sizes(h, w)
        seq_u8 = seq_u8.contiguous()
        step = 2 * self._chunk(t, h, w)          # forward() holds the two sides of a chunk at once
        chunks = [self.features(seq_u8[f0:min(t, f0 + step)]) for f0 in range(0, t, step)]
        return chunks[0] if len(chunks) == 1 else [torch.cat(c) for c in zip(*chunks)]

    def distance(self, feats_a, feats_b, per_layer=False):
        """The head on two lists of taps (features_of, or equally long slices of them along the frames):
        (n,) fp32 LPIPS on the device ((n,5) per layer), what forward() gives for the same frame pairs."""
        _, lin, _ = self._device_weights()
        if len(feats_a) != 5 or len(feats_b) != 5:
            raise ValueError('LPIPS.distance: five taps per side')
        n = feats_a[0].shape[0]
        res = torch.zeros(n, 5, dtype=torch.float32, device=feats_a[0].device)
        total = torch.zeros(n, dtype=torch.float32, device=feats_a[0].device)
        for k, (a, b) in enumerate(zip(feats_a, feats_b)):
            ops.lpips_head(a, b, lin[k], res, k, total if k == 4 else None)
        return res if per_layer else total

    def forward(self, true_u8, pred_u8, per_layer=False):
        """(t,h,w,3) uint8 device frames -> (t,) fp32 LPIPS on the device ((t,5) per layer)."""
        _, lin, _ = self._device_weights()
        for name, x in (('true', true_u8), ('pred', pred_u8)):
            if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.uint8 and x.dim() == 4 and x.shape[3] == 3):
                raise TecoganHipError(f'LPIPS: {name} must be a (t,h,w,3) uint8 device tensor, got '
                                      f'{getattr(x, "dtype", type(x))} {tuple(getattr(x, "shape", ()))}')
        if true_u8.shape != pred_u8.shape:
            raise ValueError(f'LPIPS: shapes {tuple(true_u8.shape)} / {tuple(pred_u8.shape)}')
        t, h, w, _ = true_u8.shape
        alexnet_out_sizes(h, w)
        true_u8, pred_u8 = true_u8.contiguous(), pred_u8.contiguous()
        res = torch.zeros(t, 5, dtype=torch.float32, device=true_u8.device)
        total = torch.zeros(t, dtype=torch.float32, device=true_u8.device)
        step = self._chunk(t, h, w)
        for f0 in range(0, t, step):
            f1 = min(t, f0 + step)
            nf = f1 - f0
            feats = self.features(true_u8[f0:f1], pred_u8[f0:f1])
            for k, f in enumerate(feats):
                ops.lpips_head(f[:nf], f[nf:], lin[k], res[f0:f1], k, total[f0:f1] if k == 4 else None)
        return res if per_layer else total

    __call__ = forward
