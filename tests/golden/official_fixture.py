"""Inputs of the official-protocol fixtures (tests/golden/official.npz, make_golden_official.py): integer-only
procedural clips built as lpips_fixture.clip_pair builds its own (bit-identical on every machine; the npz records
their crc32s), and the file names of the folder-level case."""
import numpy as np

from lpips_fixture import _box3, crc  # noqa: F401

# name -> (t, true (h, w), pred (h, w), distortion, seed)
CASES = {
    'a_96x128_noise8': (7, (96, 128), (96, 128), 'noise8', 21),
    'b_130x170_blur': (6, (130, 170), (128, 168), 'blur', 22),            # size-mismatch crop, then crop_8x8
    'c_vid4_576x720_noise40': (5, (576, 720), (576, 720), 'noise40', 23),  # one evaluated frame at Vid4 size
    'd0_64x96_noise8': (6, (64, 96), (64, 96), 'noise8', 24),             # the two folders of the aggregates
    'd1_64x96_blur': (7, (64, 96), (64, 96), 'blur', 25),
}
FOLDER_CASES = ('d0_64x96_noise8', 'd1_64x96_blur')
CUTFR = 2


def clip_pair(name):
    """(true, pred) uint8 (t, h, w, 3) frames of fixture case `name`."""
    t, (h, w), (ph, pw), dist, seed = CASES[name]
    rs = np.random.RandomState(seed)
    base = rs.randint(0, 256, size=(1, h + 2 * t, w + 2 * t, 3)).astype(np.int64)
    for _ in range(3):
        base = _box3(base)
    base = np.clip((base - 128) * 3 + 128, 0, 255)             # restore contrast after the blurs
    true = np.stack([base[0, i:i + h, i:i + w] for i in range(t)])   # a slow pan
    true = np.clip(true + rs.randint(-8, 9, size=true.shape), 0, 255)
    if dist == 'noise8':
        pred = true + rs.randint(-8, 9, size=true.shape)
    elif dist == 'noise40':
        pred = true + rs.randint(-40, 41, size=true.shape)
    elif dist == 'blur':
        pred = _box3(true)
    else:
        raise ValueError(dist)
    pred = np.clip(pred, 0, 255)
    if (ph, pw) != (h, w):
        pred = np.ascontiguousarray(pred[:, :ph, :pw])
    return true.astype(np.uint8), pred.astype(np.uint8)


def frame_file_names(t):
    """Names under which frame 0..t-1 of a folder case are written: numeric order differs from name order
    (frame_10 follows frame_9), so a reader that sorts by name alone mixes the frames up."""
    return [f'frame_{8 + i}.png' for i in range(t)]


# files a reader of the protocol must not pick up
DECOY_NAMES = ('IB_0001.png', 'frame_3.jpg', 'notes.txt')


def write_folder(root, name, frames, decoys=True):
    """A folder of the protocol under pathlib root: the frames as PNGs named by frame_file_names, plus files a
    reader must skip (their content differs from every frame).  Returns its path."""
    from PIL import Image
    d = root / name
    d.mkdir(parents=True)
    for fn, frame in zip(frame_file_names(len(frames)), frames):
        Image.fromarray(frame).save(str(d / fn))
    if decoys and len(frames):
        Image.fromarray(255 - frames[0]).save(str(d / 'IB_0001.png'))
        Image.fromarray(255 - frames[0]).save(str(d / 'frame_3.jpg'))
        (d / 'notes.txt').write_text('x')
    return str(d)
