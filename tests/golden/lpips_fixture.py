"""Inputs and weights of the LPIPS fixtures (tests/golden/lpips.npz, make_golden_lpips.py).

AlexNet weights are procedural, as in procedural_weights.py: numpy's frozen legacy RandomState
seeded by crc32(key name), fan-in-uniform magnitudes times a per-layer gain (the gains keep every
relu tap well populated: >= 5 % non-zeros on the fixture frames).  The real ImageNet AlexNet is
not obtainable offline; the lin weights are the reference's own v0.1 file, stored as arrays in
lpips.npz.

Frames come from integer arithmetic only (RandomState.randint, integer box blurs, integer noise,
clipping), so they are bit-identical on every machine; lpips.npz records their crc32s."""
import zlib

import numpy as np
import torch

# features index -> (cout, cin, k, gain)
ALEX_LAYERS = {0: (64, 3, 11, 1.0), 3: (192, 64, 5, 1.4), 6: (384, 192, 3, 1.4),
               8: (256, 384, 3, 1.4), 10: (256, 256, 3, 1.4)}

# name -> (t, true (h, w), pred (h, w), distortion, seed)
CASES = {
    'min64_noise2': (3, (64, 64), (64, 64), 'noise2', 11),
    'odd100x132_blur': (2, (100, 132), (100, 132), 'blur', 12),
    'vid4_576x720_noise40': (2, (576, 720), (576, 720), 'noise40', 13),
    'crop130x170_noise40': (4, (130, 170), (128, 168), 'noise40', 14),
    'odd100x132_noise2': (3, (100, 132), (100, 132), 'noise2', 15),
    'min64_noise1': (2, (64, 64), (64, 64), 'noise1', 16),
}


def _rs(name, seed=0):
    return np.random.RandomState((zlib.crc32(name.encode()) + seed) & 0x7FFFFFFF)


def alexnet_state_dict(seed=0):
    """torchvision alexnet().features key layout, fp32 (no classifier)."""
    sd = {}
    for idx, (co, ci, k, gain) in ALEX_LAYERS.items():
        b = gain / np.sqrt(ci * k * k)
        kw, kb = f'features.{idx}.weight', f'features.{idx}.bias'
        sd[kw] = torch.from_numpy(_rs(kw, seed).uniform(-b * np.sqrt(3.0), b * np.sqrt(3.0),
                                                        size=(co, ci, k, k)).astype(np.float32))
        sd[kb] = torch.from_numpy(_rs(kb, seed).uniform(-b, b, size=(co,)).astype(np.float32))
    return sd


def _box3(x):
    """Integer 3x3 box blur over (h, w) of (t, h, w, 3) int64, edge-replicated, rounded half up."""
    p = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)), mode='edge')
    h, w = x.shape[1], x.shape[2]
    s = sum(p[:, dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3))
    return (s + 4) // 9


def clip_pair(name):
    """(true, pred) uint8 (t, h, w, 3) frames of fixture case `name`."""
    t, (h, w), (ph, pw), dist, seed = CASES[name]
    rs = np.random.RandomState(seed)
    base = rs.randint(0, 256, size=(1, h + 2 * t, w + 2 * t, 3)).astype(np.int64)
    for _ in range(3):
        base = _box3(base)
    base = np.clip((base - 128) * 3 + 128, 0, 255)             # restore contrast after the blurs
    # a slow pan: frame i is the window shifted by i pixels in both directions
    true = np.stack([base[0, i:i + h, i:i + w] for i in range(t)])
    true = np.clip(true + rs.randint(-8, 9, size=true.shape), 0, 255)
    if dist == 'noise1':
        pred = true + rs.randint(-1, 2, size=true.shape)
    elif dist == 'noise2':
        pred = true + rs.randint(-2, 3, size=true.shape)
    elif dist == 'noise40':
        pred = true + rs.randint(-40, 41, size=true.shape)
    elif dist == 'blur':
        pred = _box3(true)
    else:
        raise ValueError(dist)
    pred = np.clip(pred, 0, 255)
    if (ph, pw) != (h, w):                                      # a differently sized prediction
        pred = np.ascontiguousarray(pred[:, :ph, :pw])
    return true.astype(np.uint8), pred.astype(np.uint8)


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xFFFFFFFF
