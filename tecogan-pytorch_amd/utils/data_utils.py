"""Host-side helpers mirroring codes/utils/data_utils.py for the path."""
import numpy as np


def float32_to_uint8(inputs):
    """data_utils.py:80-87 (host version, for arrays already on the CPU).
    The device path is ops.quantize_u8_hwc."""
    return np.uint8(np.clip(np.round(inputs * 255), 0, 255))


def gaussian_kernel2d(sigma, ksize=None):
    """2-D Gaussian of create_kernel (data_utils.py:11-20), one channel."""
    if ksize is None:
        ksize = 1 + 2 * int(sigma * 3.0)
    xs = np.arange(ksize, dtype=np.float64) - (ksize - 1) / 2.0
    g1 = np.exp(-0.5 * (xs / sigma) ** 2)
    g2 = np.outer(g1, g1)
    return np.float32(g2 / g2.sum())


def save_sequence(seq_dir, seq_data, frm_idx_lst=None):
    """data_utils.py:90-113: each frame of a thwc | rgb | uint8 sequence as a PNG in seq_dir
    (named by frm_idx_lst, default 0000.png, ...); written with Pillow from RGB."""
    import os
    from PIL import Image
    tot_frm = len(seq_data)
    if frm_idx_lst is None:
        frm_idx_lst = ['{:04d}.png'.format(i) for i in range(tot_frm)]
    os.makedirs(seq_dir, exist_ok=True)
    for i in range(tot_frm):
        Image.fromarray(np.ascontiguousarray(seq_data[i])).save(os.path.join(seq_dir, frm_idx_lst[i]))
