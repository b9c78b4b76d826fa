"""The 25-product identity of the resident launch's transposed-conv tail (tg_conv3x3_wino_res.hip, "tail"), restated
in fp64 exactly as the kernel states it -- the seven in-register weight sums, both +-1 data transforms, the product
numbering p = 0..24 and the output sums (phase (1,1): rows first) -- against torch's conv_transpose2d(.., 2, 1, 1).
The rehearsal that needs no device: a wrong tap, sign or product index shows here at 1e-1, not at 1e-12."""
import pytest
import torch
import torch.nn.functional as F


def tail_identity(x, w, bias):
    """x (cin, h, w) with h, w even; w (cin, cout, 3, 3); bias (cout) -> (cout, 2h, 2w), per 2x2 input tile."""
    cin, h, wd = x.shape
    cout = w.shape[1]
    xp = torch.zeros(cin, h + 1, wd + 1, dtype=x.dtype)          # the window's third row / column: ring or zero
    xp[:, :h, :wd] = x

    def W(ky, kx):
        return w[:, :, ky, kx]                                   # (cin, cout)
    # the seven sums, as the kernel forms them from the nine taps
    gx = [W(1, 2), W(1, 2) + W(1, 0), W(1, 0)]
    gy = [W(2, 1), W(2, 1) + W(0, 1), W(0, 1)]
    g0 = [W(2, 2), W(2, 2) + W(2, 0), W(2, 0)]
    g2 = [W(0, 2), W(0, 2) + W(0, 0), W(0, 0)]
    wm = [None] * 25                                             # product p -> weight matrix
    for p in range(4):
        wm[p] = W(1, 1)
    for ya in range(2):
        for j in range(3):
            wm[4 + 3 * ya + j] = gx[j]
    for i in range(3):
        for xb in range(2):
            wm[10 + 2 * i + xb] = gy[i]
    for j in range(3):
        wm[16 + j] = g0[j]
        wm[19 + j] = g0[j] + g2[j]
        wm[22 + j] = g2[j]

    out = torch.zeros(cout, 2 * h, 2 * wd, dtype=x.dtype)
    for ty in range(h // 2):
        for tx in range(wd // 2):
            d = xp[:, 2 * ty:2 * ty + 3, 2 * tx:2 * tx + 3]      # (cin, 3, 3)
            c3 = [[d[:, i, 0] - d[:, i, 1], d[:, i, 1], d[:, i, 2] - d[:, i, 1]] for i in range(3)]
            v = [None] * 25                                      # product p -> data value per input channel
            for ya in range(2):
                for xb in range(2):
                    v[2 * ya + xb] = d[:, ya, xb]
                for j in range(3):
                    v[4 + 3 * ya + j] = c3[ya][j]
            for xb in range(2):
                v[10 + xb] = d[:, 0, xb] - d[:, 1, xb]
                v[12 + xb] = d[:, 1, xb]
                v[14 + xb] = d[:, 2, xb] - d[:, 1, xb]
            for j in range(3):
                v[16 + j] = c3[0][j] - c3[1][j]
                v[19 + j] = c3[1][j]
                v[22 + j] = c3[2][j] - c3[1][j]
            m = [v[p] @ wm[p] for p in range(25)]                # the K loop: (cout,) per product
            for ya in range(2):
                s3 = [m[16 + 3 * ya + j] + m[16 + 3 * (ya + 1) + j] for j in range(3)]
                for xb in range(2):
                    o = out[:, 4 * ty + 2 * ya:4 * ty + 2 * ya + 2, 4 * tx + 2 * xb:4 * tx + 2 * xb + 2]
                    o[:, 0, 0] = m[2 * ya + xb]
                    o[:, 0, 1] = m[4 + 3 * ya + xb] + m[4 + 3 * ya + xb + 1]
                    o[:, 1, 0] = m[10 + 2 * ya + xb] + m[10 + 2 * (ya + 1) + xb]
                    o[:, 1, 1] = s3[xb] + s3[xb + 1]
    return out + bias[:, None, None]


@pytest.mark.parametrize('h,w', [(2, 2), (5, 7), (8, 24)])
def test_tail_identity_equals_conv_transpose2d(h, w):
    """Ragged shapes: an odd extent is padded to the next even one with zeros, as the resident block holds pixels
    outside the image, and the outputs past the image are dropped."""
    g = torch.Generator().manual_seed(31 + h)
    cin, cout = 8, 6
    x = torch.randn(cin, h, w, generator=g, dtype=torch.float64)
    wt = torch.randn(cin, cout, 3, 3, generator=g, dtype=torch.float64)
    b = torch.randn(cout, generator=g, dtype=torch.float64)
    he, we = h + (h & 1), w + (w & 1)
    xe = torch.zeros(cin, he, we, dtype=torch.float64)
    xe[:, :h, :w] = x
    got = tail_identity(xe, wt, b)[:, :2 * h, :2 * w]
    ref = F.conv_transpose2d(x[None], wt, b, 2, 1, 1)[0]
    assert got.shape == ref.shape
    e = (got - ref).abs().max().item()
    print('tail identity %dx%d: max error %.3g' % (h, w, e))
    assert e <= 1e-12
