"""Golden vectors of the fp16 inference mode, made with the reference network on the CPU.

Authoring container only (needs the reference tree, see _ref_import.py); the tests read the committed
tests/golden/fp16_{BD4,BI2,BD4_odd}.npz and nothing else.

The specification is applied to the reference FRNet with forward hooks:
  * the weights of srnet.conv_in.0, srnet.resblocks.*.conv.{0,2} and srnet.conv_up.0 are rounded to fp16 once;
  * SRNet's input is rounded to fp16; conv_in + ReLU, each block's inner ReLU and each block's output (after the
    skip add) are rounded to fp16; conv_up.0 reads fp16 and hands fp32 on, unrounded;
  * everything else is the reference's own fp32 code.
Three runs per clip:
  spec   the fp16 layers accumulate in float64 (the exact statement of the specification),
  alt    the same layers accumulate in torch's fp32 (an equally valid implementation),
  fp32   the plain reference.
Per clip one file with
  u8_inner        (t - 2, H, W, c) uint8 `spec`, frames 1 .. t - 2
  hr_first/last   (c, H, W) float32      `spec`, first and last frame (their uint8 frames are the quantised floats:
                                         fp16_fixture.load() rebuilds the full (t, H, W, c) uint8 clip; a committed file
                                         has to stay below 1 MiB)
  noise_rel_l2    (t,)  relL2(alt, spec)                     -- the yardstick of the whole-clip test
  noise_u8_share  (t,)  share of uint8 pixels where alt != spec
  noise_u8_max    (t,)  largest uint8 difference alt vs spec
  fp32_rel_l2, fp32_u8_share, fp32_u8_max: the same three for the plain fp32 run against spec
  scale, h, w, t, seed, degradation: the configuration (the LR clip is procedural_weights.smooth_clip(t, 3, h, w, seed))
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _ref_import  # noqa: E402
from procedural_weights import generator_state_dict, smooth_clip  # noqa: E402

CLIPS = {            # name: (scale, degradation, h, w, frames, seed)
    'BD4': (4, 'BD', 32, 48, 8, 0),
    'BI2': (2, 'BI', 64, 96, 5, 2),
    'BD4_odd': (4, 'BD', 37, 53, 5, 3),
}


def r16(t):
    """Correctly rounded to fp16 (nearest even) from fp32 or fp64, returned in the input's dtype."""
    a = t.detach().numpy()
    return torch.from_numpy(a.astype(np.float16).astype(a.dtype))


def build(ns, scale, deg):
    net = ns.nets.FRNet(3, 3, 64, 10, deg, scale)
    net.load_state_dict(generator_state_dict(scale=scale, degradation=deg), strict=False)
    return net.eval()


def hook(net, wide):
    sr = net.srnet
    mods = [sr.conv_in[0]] + [m for b in sr.resblocks for m in (b.conv[0], b.conv[2])] + [sr.conv_up[0]]
    with torch.no_grad():
        for m in mods:
            m.weight.copy_(r16(m.weight))
            if wide:
                m.double()
    up = (lambda t: t.double()) if wide else (lambda t: t)
    sr.conv_in.register_forward_pre_hook(lambda m, a: (up(r16(a[0])),))
    sr.conv_in.register_forward_hook(lambda m, a, o: r16(o))
    for b in sr.resblocks:
        b.conv[1].register_forward_hook(lambda m, a, o: r16(o))
        b.register_forward_hook(lambda m, a, o: r16(o))
    sr.conv_up[0].register_forward_hook(lambda m, a, o: o.float())


def frames(net, clip, scale):
    t, c, h, w = clip.shape
    lp, hp = torch.zeros(1, c, h, w), torch.zeros(1, c, scale * h, scale * w)
    out = []
    with torch.no_grad():
        for i in range(t):
            lc = clip[i:i + 1]
            hc = net.step(lc, lp, hp)
            lp, hp = lc, hc
            out.append(hc[0].numpy().copy())
    return np.stack(out)


def main():
    ns = _ref_import.import_reference()
    torch.set_num_threads(min(16, os.cpu_count() or 1))

    def u8(x):                                   # (t, c, H, W) float -> (t, H, W, c) uint8, the reference's quantiser
        return ns.data_utils.float32_to_uint8(np.ascontiguousarray(x.transpose(0, 2, 3, 1)))

    def dist(a, b):
        rel, share, mx = [], [], []
        ua, ub = u8(a).astype(np.int32), u8(b).astype(np.int32)
        for i in range(a.shape[0]):
            d = a[i].astype(np.float64) - b[i].astype(np.float64)
            rel.append(np.sqrt((d ** 2).sum() / (b[i].astype(np.float64) ** 2).sum()))
            du = np.abs(ua[i] - ub[i])
            share.append(float((du > 0).mean()))
            mx.append(int(du.max()))
        return np.array(rel), np.array(share), np.array(mx, dtype=np.int32)

    for name, (scale, deg, h, w, t, seed) in CLIPS.items():
        clip = smooth_clip(t, 3, h, w, seed=seed)
        plain = frames(build(ns, scale, deg), clip, scale)
        n_alt = build(ns, scale, deg); hook(n_alt, False); alt = frames(n_alt, clip, scale)
        n_spec = build(ns, scale, deg); hook(n_spec, True); spec = frames(n_spec, clip, scale)
        nr, nsh, nmx = dist(alt, spec)
        fr, fsh, fmx = dist(plain, spec)
        out = os.path.join(HERE, f'fp16_{name}.npz')
        q = u8(spec)
        from oracle import tecogan_oracle as O       # the loader's quantiser is the reference's, bit for bit
        for i in (0, -1):
            assert np.array_equal(O.float32_to_uint8(spec[i].astype(np.float32)).transpose(1, 2, 0), q[i])
        np.savez_compressed(out, u8_inner=q[1:-1], hr_first=spec[0].astype(np.float32), hr_last=spec[-1].astype(np.float32),
                            noise_rel_l2=nr, noise_u8_share=nsh, noise_u8_max=nmx,
                            fp32_rel_l2=fr, fp32_u8_share=fsh, fp32_u8_max=fmx,
                            scale=scale, h=h, w=w, t=t, seed=seed, degradation=deg)
        print(f'{name}: {os.path.getsize(out)} bytes; noise relL2 {nr.min():.2e}..{nr.max():.2e}, u8 share '
              f'{nsh.min():.4f}..{nsh.max():.4f} (max {nmx.max()}); fp32 relL2 {fr.min():.2e}..{fr.max():.2e}, '
              f'u8 share {fsh.min():.4f}..{fsh.max():.4f} (max {fmx.max()})')


if __name__ == '__main__':
    main()
