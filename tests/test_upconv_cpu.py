"""conv3x3(bilinear_x2(x)) with the channel mix at the low resolution (csrc/tg_upconv.hip), without a GPU:

  * tests/upconv_ref.py, the torch statement the GPU tests use as their reference, equals F.interpolate + F.conv2d in fp64
    to rounding, borders included -- and the bound has teeth: with every tap shifted the wrong way, or with a border that
    is not clamped, it misses the same bound by orders of magnitude;
  * the exact-arithmetic inputs of the GPU test (integers, +-1/2 weights) give the same BITS through both forms in fp32,
    which is what lets that test ask for bit equality;
  * the packed-size query and the rule's refusals (unsupported channel counts; TG_CONV_WINO=1, TG_UPCONV=0).
"""
import os
import subprocess
import sys

import pytest
import torch

import tecogan_pytorch_amd  # noqa: F401
from tecogan_pytorch_amd import _lib as L

from tests import upconv_ref as R

ROOT_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (2, 3), (5, 7), (9, 33)]
PAIRS = [(64, 32), (128, 64), (256, 128)]          # FNet's readers: flow.0, decoder3.0, decoder2.0
# fp64: products of O(1) values summed over 9 * cin <= 2304 terms, each side within a few hundred ulp of 2.2e-16
IDENTITY_TOL = 1e-12


def _case(cin, cout, h, w, dtype, seed=0):
    g = torch.Generator().manual_seed(seed + 131 * cin + 7 * h + w)
    x = (torch.rand(2, cin, h, w, generator=g, dtype=torch.float64) * 2 - 1).to(dtype)
    wt = ((torch.rand(cout, cin, 3, 3, generator=g, dtype=torch.float64) * 2 - 1) / (3 * cin ** 0.5)).to(dtype)
    b = (torch.rand(cout, generator=g, dtype=torch.float64) * 2 - 1).to(dtype)
    return x, wt, b


@pytest.mark.parametrize('h,w', SHAPES)
def test_factored_form_is_the_composed_form_in_fp64(h, w):
    for cin, cout in PAIRS:
        x, wt, b = _case(cin, cout, h, w, torch.float64)
        want = R.composed(x, wt, b, 0.2)
        e = (R.factored(x, wt, b, 0.2) - want).abs().max().item()
        print('%dx%d %d->%d: max |factored - composed| %.2e' % (h, w, cin, cout, e))
        assert e <= IDENTITY_TOL, (h, w, cin, cout, e)
        up = torch.nn.functional.interpolate(x, scale_factor=2, mode='bilinear', align_corners=False)
        assert (R.up2(x) - up).abs().max().item() <= 1e-15      # the written-out taps are F.interpolate's


@pytest.mark.parametrize('h,w', SHAPES)
def test_the_bound_has_teeth(h, w):
    """A tap shifted the wrong way and an unclamped border both miss IDENTITY_TOL by at least 1e6 x."""
    cin, cout = 64, 32
    x, wt, b = _case(cin, cout, h, w, torch.float64)
    want = R.composed(x, wt, b, 0.2)
    shifted = (R.factored(x, wt, b, 0.2, shift=-1) - want).abs().max().item()
    unclamped = (R.factored(x, wt, b, 0.2, clamp=False) - want).abs().max().item()
    print('%dx%d: shifted taps %.2e, unclamped border %.2e' % (h, w, shifted, unclamped))
    assert shifted >= 1e6 * IDENTITY_TOL, shifted
    assert unclamped >= 1e6 * IDENTITY_TOL, unclamped


def exact_inputs(cin, cout, h, w, n, weights, seed=0):
    """Integers in [-4, 4], weights +-1/2 on one tap (`weights` = 0..8) or sparse over all of them ('mixed'), small
    integer bias: every product and partial sum of either form is a multiple of 2^-5 below 2^12, exact in fp32."""
    g = torch.Generator().manual_seed(seed + 17 * cin + 3 * h + w)
    x = torch.randint(-4, 5, (n, cin, h, w), generator=g).float()
    sign = torch.randint(0, 2, (cout, cin, 3, 3), generator=g).float() - 0.5
    keep = (torch.rand(cout, cin, 3, 3, generator=g) < 0.25).float()
    wt = sign * keep
    if weights != 'mixed':
        tap = torch.zeros(3, 3)
        tap[weights // 3, weights % 3] = 1
        wt = wt * tap
    b = torch.randint(-3, 4, (cout,), generator=g).float()
    return x, wt, b


@pytest.mark.parametrize('weights', list(range(9)) + ['mixed'])
def test_exact_inputs_give_equal_bits_in_fp32(weights):
    for (h, w), (cin, cout) in zip(SHAPES, PAIRS + PAIRS[:1]):
        x, wt, b = exact_inputs(cin, cout, h, w, 2, weights)
        for slope in (None, 0.2):
            a, c = R.factored(x, wt, b, slope), R.composed(x, wt, b, slope)
            assert torch.equal(a, c), (weights, h, w, cin, cout, slope, (a - c).abs().max().item())
            if slope is None:      # ... and they are the exact values: fp64 computes the same
                assert torch.equal(a.double(), R.composed(x.double(), wt.double(), b.double()))


def test_packed_size_query_and_refusals():
    lib = L.lib()
    for cin, cout in PAIRS:
        assert lib.tg_upconv_packed_floats(cin, cout) == 9 * cin * cout
    for cin, cout in [(64, 64), (32, 16), (96, 48), (256, 64), (0, 0), (128, 32), (512, 256)]:
        assert lib.tg_upconv_packed_floats(cin, cout) == 0, (cin, cout)
        assert lib.tg_upconv_prefers(8, cin, cout, 64, 160) == 0, (cin, cout)
        assert lib.tg_upconv_pack(1 << 12, 1 << 12, cin, cout, 0, None) == L.TG_E_ARG      # refused before any launch
    assert lib.tg_upconv_pack(None, None, 64, 32, 0, None) == L.TG_E_ARG
    assert lib.tg_upconv_pack(1 << 12, 1 << 12, 64, 32, 16, None) == L.TG_E_ARG
    for n, h, w in [(0, 8, 8), (8, 0, 8), (8, 8, 0)]:
        assert lib.tg_upconv_prefers(n, 64, 32, h, w) == 0


FLAGSHIP = [(256, 128, 16, 40), (128, 64, 32, 80), (64, 32, 64, 160)]      # the readers' source maps at 134x320


def _prefers_in_child(env):
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from tecogan_pytorch_amd import _lib as L\n"
            "print(' '.join(str(L.lib().tg_upconv_prefers(8, ci, co, h, w)) for ci, co, h, w in %r))\n" % (ROOT_DIR, FLAGSHIP))
    full = {k: v for k, v in os.environ.items() if k not in ('TG_UPCONV', 'TG_CONV_WINO')}
    full.update(env)
    r = subprocess.run([sys.executable, '-c', code], env=full, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return [int(v) for v in r.stdout.split()]


def test_default_rule_picks_the_flagship_pass_and_nothing_smaller():
    """The rule as measured (EXPERIMENTS.md): the three readers at a 134x320 frame's source maps, batched passes of 2 to 8
    pairs; not the one-pair frame plan, not a smaller map (the frame plans the tests run keep the composed launches)."""
    if 'TG_UPCONV' in os.environ or os.environ.get('TG_CONV_WINO') == '1':
        assert _prefers_in_child({}) == [1, 1, 1]
        return
    lib = L.lib()
    for cin, cout, h, w in FLAGSHIP:
        for n in range(2, 9):
            assert lib.tg_upconv_prefers(n, cin, cout, h, w) == 1, (n, cin, h, w)
        assert lib.tg_upconv_prefers(1, cin, cout, h, w) == 0
        assert lib.tg_upconv_prefers(8, cin, cout, h, w - 1) == 0
        assert lib.tg_upconv_prefers(8, cin, cout, 2 * h, 2 * w) == 1
    for cin, cout, h, w in [(256, 128, 8, 20), (128, 64, 16, 40), (64, 32, 32, 80)]:      # 8 pairs of 64x160
        assert lib.tg_upconv_prefers(8, cin, cout, h, w) == 0


def test_rule_switches():
    assert _prefers_in_child({'TG_CONV_WINO': '1'}) == [0, 0, 0]
    assert _prefers_in_child({'TG_CONV_WINO': '1', 'TG_UPCONV': '1'}) == [0, 0, 0]
    assert _prefers_in_child({'TG_UPCONV': '0'}) == [0, 0, 0]
    assert _prefers_in_child({'TG_UPCONV': '1'}) == [1, 1, 1]
