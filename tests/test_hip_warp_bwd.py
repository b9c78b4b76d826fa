"""backward_warp_bwd_kernel (csrc/tg_train.hip: tg_backward_warp_bwd, _acc, _s2d_bwd) against float64 autograd of the
oracle's backward_warp at EVERY pixel, on every entry point and every geometry of the launch (64 columns x 4 rows per
block, blockIdx.z = n).  The flows come from tests/tape_ref.py: kinkfree_flow -- every sampling position is at least
1/8 pixel from an integer and from the clip limits, clipped positions at least 1/2 pixel outside -- so the fp32
kernel and the float64 reference take every floor / clip decision alike and no pixel has to be left out.

Bounds (u = 2^-24, gamma_k = k u / (1 - k u) from tests/train_reductions_ref.py; none comes from a kernel's output):

  position   `sx` is reached from `flow` by POS_OPS = 4 rounded operations (fx / halfx, + linspace, + 1.0f, * halfx;
             tape_ref.py lists them next to the kernel lines), each worth at most u (size - 1):
             delta = 4 u (size - 1) along that axis.
  d/dflow    |got - ref64| <= gamma_k S + delta S2 with k = 7 c + 1 (tape_ref.flow_chain: 1.f - wy1, then per channel
             two differences, two products, their sum, the product with g and the accumulation), S the per-pixel sum
             of absolute terms of the formula and S2 = sum_ch |g| (|v01 - v00| + |v11 - v10|) (the x component
             depends on the position along y only, through wy; delta is that axis's).  Exactly 0.0 where clipped.
  d/dimg     |got - ref64| <= gamma_(m + 3) A + sens: m contributions g * wy * wx of at most 4 roundings each meet
             in m - 1 atomic additions of free order; A their absolute sum, sens the scatter of
             |g| (wy delta_x + wx delta_y).  Onto a non-zero pre-fill p: gamma_(m + 4) (A + |p|) + sens.  Elements
             that no pixel samples are exactly 0.0 / exactly the pre-fill.

Each check prints a `[measured]` line (worst error and its bound); run with -s to see them."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import tape_ref as TR

SENTINEL = 12345.0


@pytest.fixture(scope='module')
def ops():
    import tecogan_pytorch_amd.ops as ops_
    return ops_


def dev(t):
    return t.cuda().contiguous()


@functools.lru_cache(maxsize=None)
def case(shape, out_frac, s2d):
    """Inputs and the float64 reference of one case: computed once, shared, never modified."""
    x, flow, dy, cx, cy = TR.warp_inputs(11, shape, out_frac, s2d)
    ref = TR.warp_bwd_ref(x, flow, dy, s2d)
    assert torch.equal(ref.clip_x, cx) and torch.equal(ref.clip_y, cy)
    return x, flow, dy, ref


def check(name, got, ref, bound, exact=None, exact_value=None):
    """|got - ref| <= bound at every element; where `exact`, got == exact_value bit for bit."""
    got = got.detach().cpu().double()
    assert got.shape == ref.shape and torch.isfinite(got).all(), name
    err = (got - ref).abs()
    ratio = (err / bound.clamp_min(1e-300)).reshape(-1)
    i = int(ratio.argmax())
    print(f'[measured] {name}: err {err.reshape(-1)[i].item():.3e} bound {bound.reshape(-1)[i].item():.3e} '
          f'({ratio[i].item():.3f} of it); max err {err.max().item():.3e}, scale {ref.abs().max().item():.3e}')
    assert (err <= bound).all(), f'{name}: {int((err > bound).sum())} elements past their bound, worst at {i}'
    if exact is not None:
        want = torch.broadcast_to(torch.as_tensor(exact_value, dtype=torch.float64), got.shape)
        assert torch.equal(got[exact], want[exact]), f'{name}: {int((got[exact] != want[exact]).sum())} elements not exact'


def check_flow(name, dflow, ref, shape):
    n, c, h, w = shape
    bx, by = TR.flow_bound(ref, c, h, w)
    check(name + ' d/dfx', dflow[:, 0], ref.dflow[:, 0], bx, ref.clip_x, 0.0)
    check(name + ' d/dfy', dflow[:, 1], ref.dflow[:, 1], by, ref.clip_y, 0.0)


def check_img(name, dimg, ref, prefill=None):
    want = ref.dimg if prefill is None else ref.dimg + prefill.double()
    check(name + ' d/dimg', dimg, want, TR.img_bound(ref, prefill), ref.count == 0,
          0.0 if prefill is None else prefill.double())


def prefill_for(shape):
    return torch.from_numpy(np.random.RandomState(23).uniform(0.5, 2.0, shape).astype(np.float32))


PLAIN = [(s, TR.OUT_FRAC) for s in TR.WARP_SHAPES] + [((2, 3, 17, 23), 1.0), ((2, 3, 17, 23), 0.0)]


@pytest.mark.parametrize('shape,out_frac', PLAIN)
def test_plain(ops, shape, out_frac):
    x, flow, dy, ref = case(shape, out_frac, 1)
    dimg, dflow = ops.backward_warp_bwd(dev(x), dev(flow), dev(dy))
    name = f'plain {shape} out {out_frac}'
    check_flow(name, dflow, ref, shape)
    check_img(name, dimg, ref)
    if out_frac >= 1.0:
        assert not dflow.any()                               # every pixel clipped on both axes


@pytest.mark.parametrize('shape,out_frac', PLAIN)
def test_accumulate_onto_a_prefilled_gradient(ops, shape, out_frac):
    x, flow, dy, ref = case(shape, out_frac, 1)
    pre = prefill_for(shape)
    acc = dev(pre).clone()
    dimg, dflow = ops.backward_warp_bwd(dev(x), dev(flow), dev(dy), dimg_acc=acc)
    assert dimg.data_ptr() == acc.data_ptr()
    name = f'acc {shape} out {out_frac}'
    check_flow(name, dflow, ref, shape)
    check_img(name, acc, ref, pre)


@pytest.mark.parametrize('shape,s2d', [((2, 3, 18, 70), 2), ((1, 3, 8, 132), 4), ((1, 3, 8, 132), 2), ((1, 1, 2, 2), 2)])
@pytest.mark.parametrize('accumulate', [False, True])
def test_space_to_depth_layout(ops, shape, s2d, accumulate):
    x, flow, dy, ref = case(shape, TR.OUT_FRAC, s2d)
    pre = prefill_for(shape) if accumulate else None
    acc = dev(pre).clone() if accumulate else None
    dimg, dflow = ops.backward_warp_bwd(dev(x), dev(flow), dev(dy), dimg_acc=acc, s2d=s2d)
    name = f's2d {s2d} {shape} acc {accumulate}'
    check_flow(name, dflow, ref, shape)
    check_img(name, dimg, ref, pre)
    if accumulate:
        assert dimg.data_ptr() == acc.data_ptr()


@pytest.mark.parametrize('shape,s2d', [((2, 3, 17, 23), 1), ((2, 3, 18, 70), 1), ((2, 3, 18, 70), 2)])
def test_one_gradient_only(ops, shape, s2d):
    x, flow, dy, ref = case(shape, TR.OUT_FRAC, s2d)
    dimg, dflow = ops.backward_warp_bwd(dev(x), dev(flow), dev(dy), need_img=False, s2d=s2d)
    assert dimg is None
    check_flow(f'flow only {shape} s2d {s2d}', dflow, ref, shape)
    dimg, dflow = ops.backward_warp_bwd(dev(x), dev(flow), dev(dy), need_flow=False, s2d=s2d)
    assert dflow is None
    check_img(f'image only {shape} s2d {s2d}', dimg, ref)


@pytest.mark.parametrize('shape,s2d,accumulate', [((2, 3, 17, 23), 1, False), ((2, 3, 18, 70), 1, True),
                                                  ((2, 3, 18, 70), 2, False), ((1, 3, 8, 132), 4, True)])
def test_flow_gradient_into_a_slice_of_a_larger_buffer(ops, shape, s2d, accumulate):
    """dflow_out: the middle slice of a frame-major buffer; the slices around it keep their sentinel."""
    n, c, h, w = shape
    x, flow, dy, ref = case(shape, TR.OUT_FRAC, s2d)
    big = torch.full((3, n, 2, h, w), SENTINEL, dtype=torch.float32, device='cuda')
    pre = prefill_for(shape) if accumulate else None
    acc = dev(pre).clone() if accumulate else None
    dimg, dflow = ops.backward_warp_bwd(dev(x), dev(flow), dev(dy), dflow_out=big[1], dimg_acc=acc, s2d=s2d)
    assert dflow.data_ptr() == big[1].data_ptr()
    assert (big[0] == SENTINEL).all() and (big[2] == SENTINEL).all()
    name = f'slice {shape} s2d {s2d} acc {accumulate}'
    check_flow(name, big[1], ref, shape)
    check_img(name, dimg, ref, pre)
