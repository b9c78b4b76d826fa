"""The reference's PNG-folder test sets (codes/data/paired_folder_dataset.py:16-63,
unpaired_folder_dataset.py:16-52, utils/base_utils.py:114-138), decoded with Pillow.

`gt_seq_dir/<key>/...` holds one sequence per key (frames found recursively, sorted, png | jpg);
with `lr_seq_dir` the sequences are paired (keys present in both), without it the LR frames are made
from the GT on the device (prepare_inference_data): by the BD degradation, or -- for an entry with `on_device: true` --
by the BI degradation.  `filter_file` (one key per line) or
`filter_list` selects keys."""
import os
import os.path as osp

import numpy as np
import torch


def retrieve_files(dir, suffix='png|jpg'):
    """Files with one of the suffixes under dir and its sub-directories, sorted by full path."""
    if not dir:
        return []
    if isinstance(suffix, str):
        suffix = suffix.split('|')
    exts = ['.' + s for s in suffix]
    file_lst = []

    def walk(d):
        for name in sorted(os.listdir(d)):
            dd = osp.join(d, name)
            if osp.isdir(dd):
                walk(dd)
            elif osp.splitext(name)[-1].lower() in exts:
                file_lst.append(dd)
    walk(dir)
    file_lst.sort()
    return file_lst


def read_rgb(path):
    """hwc | rgb | uint8 (cv2.imread(path)[..., ::-1] of the reference)."""
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert('RGB'), dtype=np.uint8)


class FolderDataset:
    def __init__(self, data_opt, degradation='BD'):
        self.gt_seq_dir = data_opt['gt_seq_dir']
        self.lr_seq_dir = data_opt.get('lr_seq_dir') or None
        if degradation not in ('BD', 'BI'):
            raise ValueError(f'Unrecognized degradation type: {degradation}')
        # BI sets are paired unless the entry opts in to LR frames made from the GT on the device (`on_device: true`;
        # main.folder_test_sets hands down dataset.degradation.on_device): DESIGN.md section 7g
        if self.lr_seq_dir is None and degradation == 'BI' and not data_opt.get('on_device', False):
            raise ValueError('"lr_seq_dir" is required for BI mode (or "on_device": true, to make the LR frames from '
                             'the GT by the BI degradation on the device)')
        keys = set(os.listdir(self.gt_seq_dir))
        if self.lr_seq_dir is not None:
            keys &= set(os.listdir(self.lr_seq_dir))
        sel = keys
        if data_opt.get('filter_file') is not None:
            with open(data_opt['filter_file'], 'r') as f:
                sel = {line.strip() for line in f}
        elif data_opt.get('filter_list') is not None:
            sel = {str(k) for k in data_opt['filter_list']}
        self.keys = sorted(sel & keys)

    def __len__(self):
        return len(self.keys)

    def __getitem__(self, item):
        key = self.keys[item]
        gt = np.stack([read_rgb(p) for p in retrieve_files(osp.join(self.gt_seq_dir, key))])
        out = {'gt': torch.from_numpy(np.ascontiguousarray(gt)), 'seq_idx': key,
               'frm_idx': sorted(os.listdir(osp.join(self.gt_seq_dir, key)))}
        if self.lr_seq_dir is not None:
            lr = np.stack([read_rgb(p).astype(np.float32) / 255.0
                           for p in retrieve_files(osp.join(self.lr_seq_dir, key))])
            out['lr'] = torch.from_numpy(np.ascontiguousarray(lr))
        return out

    def __iter__(self):
        for i in range(len(self)):
            yield self[i]
