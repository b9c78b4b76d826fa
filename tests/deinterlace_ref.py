"""The specification of the motion-adaptive deinterlacer in numpy, vectorised per row.  Imports
nothing from the package: the device kernel, ops.deinterlace and the stream are compared with what this file gives.

A frame holds two fields; p = 0 is the earlier one.  tff: the earlier field owns the even rows.  par = p ^ (0 if tff else
1) is the parity of the rows the field owns.  Every plane is treated alike.  Owned rows are copied.  A missing row r has
a = cur[ra], b = cur[rb] with ra = r-1 (r+1 at the top border), rb = r+1 (r-1 at the bottom border); every x index is
clamped into the plane.  For d in (0, -1, +1): score_d = sum_{e in -1,0,1} |a[x+d+e] - b[x-d+e]|, candidate
(a[x+d] + b[x-d] + 1) >> 1; sp is the candidate of the smallest score, a later d wins only when strictly smaller.  With no
frame before: out = sp.  Else tp = the sample at (r, x) of the field one back in time (cur[r] for p = 1, prev[r] for
p = 0), m = max(|a[x] - prev[ra][x]|, |b[x] - prev[rb][x]|), out = min(max(sp, tp - m), tp + m)."""
import numpy as np

SUBSAMPLING = {'420': (2, 2), '422': (2, 1), '444': (1, 1)}
DIRECTIONS = (0, -1, 1)


def plane_shapes(h, w, chroma):
    sx, sy = SUBSAMPLING[chroma]
    c = ((h + sy - 1) // sy, (w + sx - 1) // sx)
    return [(h, w), c, c]


def frame_samples(h, w, chroma):
    return sum(a * b for a, b in plane_shapes(h, w, chroma))


def split(frame, h, w, chroma):
    """(Y, U, V) views of one frame of samples."""
    out, at = [], 0
    for ph, pw in plane_shapes(h, w, chroma):
        out.append(frame[at:at + ph * pw].reshape(ph, pw))
        at += ph * pw
    return out


def _at(row, idx):
    return row[np.clip(idx, 0, row.shape[0] - 1)]


def spatial_row(a, b, stats=None):
    """sp of one missing row from the rows above and below (int64 arrays).  stats (a dict) counts how often each
    direction wins and how often either clamp bound is used."""
    pw = a.shape[0]
    x = np.arange(pw)
    best = sp = pick = None
    for d in DIRECTIONS:
        score = sum(np.abs(_at(a, x + d + e) - _at(b, x - d + e)) for e in (-1, 0, 1))
        cand = (_at(a, x + d) + _at(b, x - d) + 1) >> 1
        if best is None:
            best, sp, pick = score, cand, np.zeros(pw, np.int64)
        else:
            take = score < best
            best, sp, pick = np.where(take, score, best), np.where(take, cand, sp), np.where(take, d, pick)
    if stats is not None:
        for d in DIRECTIONS:
            stats['dir', d] = stats.get(('dir', d), 0) + int((pick == d).sum())
    return sp


def field_plane(cur, prev, par, later, stats=None, parts=None):
    """One plane of the output frame of a field: cur, prev (None: no frame before) are (ph, pw) integer planes already
    bounded by the depth; par the parity of the owned rows; later: the field is the frame's second one (p = 1).
    parts (a list) receives (r, sp, tp, m) of every missing row that has a frame before."""
    cur = cur.astype(np.int64)
    prev = None if prev is None else prev.astype(np.int64)
    ph = cur.shape[0]
    out = cur.copy()
    for r in range(ph):
        if r % 2 == par:
            continue
        ra = r - 1 if r - 1 >= 0 else r + 1
        rb = r + 1 if r + 1 < ph else r - 1
        a, b = cur[ra], cur[rb]
        sp = spatial_row(a, b, stats)
        if prev is None:
            out[r] = sp
            continue
        tp = cur[r] if later else prev[r]
        m = np.maximum(np.abs(a - prev[ra]), np.abs(b - prev[rb]))
        lo, hi = tp - m, tp + m
        res = np.minimum(np.maximum(sp, lo), hi)
        if stats is not None:
            stats['lo'] = stats.get('lo', 0) + int((sp < lo).sum())
            stats['hi'] = stats.get('hi', 0) + int((sp > hi).sum())
            stats['sp'] = stats.get('sp', 0) + int((res == sp).sum())
            stats['n'] = stats.get('n', 0) + res.size
        if parts is not None:
            parts.append((r, sp, tp, m))
        out[r] = res
    return out


def deinterlace(frames, h, w, chroma='420', depth=8, tff=True, prev=None, first_field=0, step=1, cnt=None, stats=None):
    """frames (k, samples) uint8 | uint16 interlaced frames, prev one frame (samples,) or None -> (cnt, samples)
    progressive frames: output j is field first_field + j * step counted from frames[0].  cnt None: every field to the
    end of the clip."""
    frames = np.asarray(frames)
    k = frames.shape[0]
    if cnt is None:
        cnt = (2 * k - first_field + step - 1) // step
    top = (1 << depth) - 1
    bound = lambda f: None if f is None else np.minimum(np.asarray(f), top)
    out = np.empty((cnt, frames.shape[1]), frames.dtype)
    for j in range(cnt):
        f = first_field + j * step
        t, p = f // 2, f % 2
        assert t < k, 'field window outside the frames'
        par = p ^ (0 if tff else 1)
        cur = split(bound(frames[t]), h, w, chroma)
        before = bound(frames[t - 1] if t > 0 else prev)
        before = [None] * 3 if before is None else split(before, h, w, chroma)
        out[j] = np.concatenate([field_plane(c, b, par, p == 1, stats).reshape(-1) for c, b in zip(cur, before)])
    return out


def stream(frames, h, w, chroma='420', depth=8, tff=True, rate='field'):
    """The progressive frames of a whole cold stream: two per input frame at rate 'field', the earlier field's at 'frame'."""
    return deinterlace(frames, h, w, chroma, depth, tff, None, 0, 1 if rate == 'field' else 2)


def window(i0, cnt, rate='field'):
    """Restated from the issue, for the tests of the engine's own mapping: output frames i0 .. i0 + cnt - 1 need the input
    frames lo .. hi (lo = -1: none before) and start at field first_field of frame lo + 1."""
    if rate == 'field':
        return i0 // 2 - 1, (i0 + cnt - 1) // 2, i0 & 1
    return i0 - 1, i0 + cnt - 1, 0
