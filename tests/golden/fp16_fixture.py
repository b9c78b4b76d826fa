"""Shared pieces of the fp16-mode tests (tests/test_fp16_cpu.py, tests/test_hip_fp16.py): the loader of
tests/golden/fp16_*.npz (made by make_golden_fp16.py from the reference network), a torch-CPU restatement of
the specification built from oracle/tecogan_oracle.py's functions, and the per-layer float64 reference with
the derived error bound.  CPU only; nothing here touches the library."""
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import tecogan_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
CLIPS = ('BD4', 'BI2', 'BD4_odd')
F16_MAX = 65504.0


def load(name):
    """dict of the golden file with the full uint8 clip under 'u8' (first / last frame = the quantised floats)."""
    g = dict(np.load(os.path.join(HERE, f'fp16_{name}.npz')))
    first = O.float32_to_uint8(g['hr_first']).transpose(1, 2, 0)[None]
    last = O.float32_to_uint8(g['hr_last']).transpose(1, 2, 0)[None]
    g['u8'] = np.concatenate([first, g['u8_inner'], last], 0)
    for k in ('scale', 'h', 'w', 't', 'seed'):
        g[k] = int(g[k])
    g['degradation'] = str(g['degradation'])
    return g


def r16(t):
    """Round to fp16 (nearest even, ONE rounding also from float64: numpy's conversion; torch's float64 -> float16
    goes through float32 and rounds twice), keep the dtype."""
    a = t.detach().numpy()
    return torch.from_numpy(a.astype(np.float16).astype(a.dtype))


def body_keys(sd_srnet):
    """Weight keys of the fp16 layers in order: conv_in.0, resblocks.*.conv.{0,2}, conv_up.0."""
    nb = 1 + max(int(k.split('.')[1]) for k in sd_srnet if k.startswith('resblocks.'))
    keys = ['conv_in.0']
    for b in range(nb):
        keys += [f'resblocks.{b}.conv.0', f'resblocks.{b}.conv.2']
    return keys + ['conv_up.0'], nb


def srnet_forward_fp16(sd, lr_curr, hr_prev_tran, scale, degradation, wide):
    """O.srnet_forward with the specification's rounding points.  wide: the fp16 layers accumulate in float64
    (`spec`), else in torch's fp32 (`alt`).  sd: the keys below `srnet.`."""
    keys, nb = body_keys(sd)
    acc = torch.float64 if wide else torch.float32
    wt = {k: r16(sd[k + '.weight']).to(acc) for k in keys}
    bs = {k: sd[k + '.bias'].to(acc) for k in keys}
    conv = lambda x, k: F.conv2d(x, wt[k], bs[k], padding=1)
    x = r16(torch.cat([lr_curr, hr_prev_tran], 1)).to(acc)
    out = r16(torch.relu(conv(x, 'conv_in.0')))
    for b in range(nb):
        t = r16(torch.relu(conv(out, f'resblocks.{b}.conv.0')))
        out = r16(conv(t, f'resblocks.{b}.conv.2') + out)
    out = torch.relu(F.conv_transpose2d(out, wt['conv_up.0'], bs['conv_up.0'], stride=2, padding=1,
                                        output_padding=1).float())
    if scale == 4:
        out = torch.relu(F.conv_transpose2d(out, sd['conv_up.2.weight'], sd['conv_up.2.bias'], stride=2, padding=1,
                                            output_padding=1))
    out = F.conv2d(out, sd['conv_out.weight'], sd['conv_out.bias'], padding=1)
    return out + O.upsample(lr_curr, scale, degradation)


def frnet_step_fp16(sd, lr_curr, lr_prev, hr_prev, scale, degradation, wide):
    """O.frnet_step with the fp16 SRNet body; everything in front of SRNet is the oracle's fp32 code."""
    h, w = lr_curr.shape[2:]
    lr_flow = O.fnet_forward(O._sub(sd, 'fnet.'), lr_curr, lr_prev)
    lr_flow_pad = O.reflect_pad_br(lr_flow, h - h // 8 * 8, w - w // 8 * 8)
    hr_flow = scale * O.upsample(lr_flow_pad, scale, degradation)
    s2d = O.space_to_depth(O.backward_warp(hr_prev, hr_flow), scale)
    return srnet_forward_fp16(O._sub(sd, 'srnet.'), lr_curr, s2d, scale, degradation, wide)


def infer_fp16(sd, clip, scale, degradation, wide):
    """(t, c, h, w) -> float frames (t, c, H, W), zero initial state."""
    t, c, h, w = clip.shape
    lp, hp = torch.zeros(1, c, h, w), torch.zeros(1, c, scale * h, scale * w)
    out = []
    with torch.no_grad():
        for i in range(t):
            hc = frnet_step_fp16(sd, clip[i:i + 1], lp, hp, scale, degradation, wide)
            lp, hp = clip[i:i + 1], hc
            out.append(hc[0].numpy().copy())
    return np.stack(out)


def rel_l2(a, b):
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    return float(np.sqrt((d ** 2).sum() / (np.asarray(b, np.float64) ** 2).sum()))


def u8_diff(a, b):
    """(share of differing uint8 values, largest difference)."""
    d = np.abs(np.asarray(a).astype(np.int32) - np.asarray(b).astype(np.int32))
    return float((d > 0).mean()), int(d.max())


# ---- per layer: float64 reference and the derived bound ------------------------------------------------------

def layer_ref(x_nchw, w, bias, relu, res=None, transposed=False):
    """x_nchw, w, res: tensors whose values are exactly fp16-representable; bias fp32.  Returns float64
    (E, S): E the layer in float64, S the same sum over absolute values (sum |x w| + |bias| + |res|)."""
    xd, wd, bd = x_nchw.double(), w.double(), bias.double()
    if transposed:
        E = F.conv_transpose2d(xd, wd, bd, stride=2, padding=1, output_padding=1)
        S = F.conv_transpose2d(xd.abs(), wd.abs(), bd.abs(), stride=2, padding=1, output_padding=1)
    else:
        E = F.conv2d(xd, wd, bd, padding=1)
        S = F.conv2d(xd.abs(), wd.abs(), bd.abs(), padding=1)
    if relu:
        E = torch.relu(E)
    if res is not None:
        E = E + res.double()
        S = S + res.double().abs()
    return E, S


K_PADDED = 9 * 64        # the kernels sum 9 taps x 64 (zero padded) input channels


def bound_f16_out(E, S, k=K_PADDED):
    """|y - E| allowed for an fp16-output layer: half an fp16 ulp for the one final rounding, the standard bound of an
    fp32 sum of k exact products (+ bias, + skip) in any order, and the smallest normal fp16 (so that the test does not
    depend on how fp16 subnormals are treated)."""
    return 2.0 ** -11 * E.abs() + (k + 2) * 2.0 ** -24 * S + 2.0 ** -14


def bound_f32_out(E, S, k=K_PADDED):
    """|y - E| allowed for the fp32-output transposed convolution."""
    return (k + 3) * 2.0 ** -24 * S
