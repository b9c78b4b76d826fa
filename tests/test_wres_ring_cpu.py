"""The resident launch's hand-over geometry (tg_conv3x3_wino_res.hip: the per-workgroup ring table, filled once per
launch from wres_ring_item) against a numpy restatement, on the host: tg_conv3x3_wino_resident_ring_item is the same
function the kernel tabulates.

The restatement does not repeat the fetch side's arithmetic.  It builds the PUBLISH side's map -- which image pixel a
block stores under which of its 64 slots (`pub` in the kernel: top row 2 tx.., bottom row WR_BW + .., left column
2 WR_BW + row, right column 2 WR_BW + WR_BH + row, live tiles only) -- and requires that the (owner, slot) the fetch
side names for a ring pixel is a slot under which exactly that pixel is published."""
import ctypes as C

import numpy as np
import pytest

BH, BW, RS, NRING = 8, 24, 28, 68
SHAPES = [(8, 24), (16, 48), (24, 72), (10, 26), (26, 70), (30, 50), (134, 320)]


@pytest.fixture(scope='module')
def lib():
    from tecogan_pytorch_amd import _lib
    return _lib.lib()


def ring_item(lib, h, w, block, pi):
    o, s, d = C.c_int(-7), C.c_int(-7), C.c_int(-7)
    rc = lib.tg_conv3x3_wino_resident_ring_item(h, w, block, pi, C.addressof(o), C.addressof(s), C.addressof(d))
    return rc, o.value, s.value, d.value


def ring_pixels():
    """(ry, rx) inside the 10 x 26 window of a block for ring pixel 0..67: top row, bottom row, left and right column."""
    top = [(0, x) for x in range(BW + 2)]
    bottom = [(BH + 1, x) for x in range(BW + 2)]
    left = [(y, 0) for y in range(1, BH + 1)]
    right = [(y, BW + 1) for y in range(1, BH + 1)]
    return top + bottom + left + right


def published(h, w):
    """{(block, slot): (gy, gx)}: what the publish side stores -- per live 2 x 2 tile (ty, tx) of a block, pixel (i, j)."""
    nbx, nby = -(-w // BW), -(-h // BH)
    out = {}
    for by in range(nby):
        for bx in range(nbx):
            for ty in range(BH // 2):
                for tx in range(BW // 2):
                    gy0, gx0 = by * BH + 2 * ty, bx * BW + 2 * tx
                    if gy0 >= h or gx0 >= w:
                        continue
                    pubs = []
                    if ty == 0:
                        pubs += [(2 * tx, 0, 0), (2 * tx + 1, 0, 1)]
                    if ty == BH // 2 - 1:
                        pubs += [(BW + 2 * tx, 1, 0), (BW + 2 * tx + 1, 1, 1)]
                    if tx == 0:
                        pubs += [(2 * BW + 2 * ty, 0, 0), (2 * BW + 2 * ty + 1, 1, 0)]
                    if tx == BW // 2 - 1:
                        pubs += [(2 * BW + BH + 2 * ty, 0, 1), (2 * BW + BH + 2 * ty + 1, 1, 1)]
                    for slot, i, j in pubs:
                        key = (by * nbx + bx, slot)
                        assert key not in out
                        out[key] = (gy0 + i, gx0 + j)
    return out


@pytest.mark.parametrize('h,w', SHAPES)
def test_ring_item_against_the_publish_side(lib, h, w):
    nbx, nby = -(-w // BW), -(-h // BH)
    pub = published(h, w)
    rp = ring_pixels()
    assert len(rp) == NRING
    interior = np.zeros((BH + 2, RS), bool)
    interior[1:BH + 1, 1:BW + 1] = True
    n_valid = 0
    for block in range(nbx * nby):
        by, bx = divmod(block, nbx)
        seen = set()
        for pi, (ry, rx) in enumerate(rp):
            rc, owner, slot, lds = ring_item(lib, h, w, block, pi)
            gy, gx = by * BH - 1 + ry, bx * BW - 1 + rx
            inside = 0 <= gy < h and 0 <= gx < w
            assert rc == (1 if inside else 0), (block, pi)          # invalid <=> the pixel lies outside the image
            # the LDS cell: this ring pixel's, in the ring and not in the block's interior, no two alike
            assert lds == ry * RS + rx and 0 <= lds < (BH + 2) * RS, (block, pi)
            assert not interior[lds // RS, lds % RS] and lds % RS < BW + 2, (block, pi)
            assert lds not in seen
            seen.add(lds)
            if not inside:
                assert (owner, slot) == (-1, -1)
                continue
            n_valid += 1
            assert owner == (gy // BH) * nbx + gx // BW and owner != block, (block, pi)     # the block that contains it
            assert 0 <= slot < 64 and pub.get((owner, slot)) == (gy, gx), (block, pi, owner, slot)
            # ... and the side that faces this block: our top ring is the owner's bottom row, and so on
            ly, lx = gy % BH, gx % BW
            want = BW + lx if ry == 0 else lx if ry == BH + 1 else 2 * BW + BH + ly if rx == 0 else 2 * BW + ly
            assert slot == want, (block, pi)
    if (h, w) == (8, 24):
        assert n_valid == 0                                          # one block: nothing to fetch
    if (h, w) == (24, 72):
        assert sum(ring_item(lib, h, w, 4, pi)[0] for pi in range(NRING)) == NRING     # the centre block: all eight neighbours
        assert {ring_item(lib, h, w, 4, pi)[1] for pi in range(NRING)} == {0, 1, 2, 3, 5, 6, 7, 8}


def test_ring_item_refuses_bad_arguments(lib):
    from tecogan_pytorch_amd import _lib
    o = C.c_int(0)
    p = C.addressof(o)
    f = lib.tg_conv3x3_wino_resident_ring_item
    assert f(16, 48, 0, 0, p, p, p) in (0, 1)
    for h, w in [(0, 48), (16, 0), (-2, 48), (15, 48), (16, 47)]:
        assert f(h, w, 0, 0, p, p, p) == _lib.TG_E_SHAPE
    for block, pi in [(-1, 0), (4, 0), (0, -1), (0, NRING)]:
        assert f(16, 48, block, pi, p, p, p) == _lib.TG_E_ARG
    for args in [(None, p, p), (p, None, p), (p, p, None)]:
        assert f(16, 48, 0, 0, *args) == _lib.TG_E_ARG
    assert b'ring_item' in lib.tg_last_error_string()
