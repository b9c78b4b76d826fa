"""The resident SRNet launch's transposed-conv tail in the Winograd domain (tg_conv3x3_wino_res.hip, "tail": 25
products per tile and K step instead of 36) and conv_in's K loop without the steps over channels that do not exist.

The tail is bounded as before the change: 3e-6 of the output scale against fp64 and against the stand-alone
transposed-conv kernel (fp32 products of K = 576 in another summation order; the +-1 transforms add one rounding to
an operand).  The body stays bit-identical to the per-layer Winograd launches."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    import tecogan_pytorch_amd.ops as ops_
    from tecogan_pytorch_amd import _lib
    _lib.lib()
    return ops_


def dev(x):
    return x.cuda().contiguous()


class Body:
    """conv_in (c1 channels of one source + the rest of a second, or one source) + nb residual blocks: the per-layer
    launches into (A1, B1) and the resident launch into (A2, B2), as tests/test_hip_parity.py builds them."""

    def __init__(self, ops, h, w, nb, cin0=51, c1=3, seed=29):
        g = torch.Generator().manual_seed(seed)
        self.ops, self.h, self.w = ops, h, w
        self.lr = dev(torch.rand(1, c1, h, w, generator=g))
        self.s2d = dev(torch.rand(1, cin0 - c1, h, w, generator=g)) if cin0 > c1 else None
        ws = [dev(torch.randn(64, cin0, 3, 3, generator=g) * 0.04)] + \
             [dev(torch.randn(64, 64, 3, 3, generator=g) * 0.03) for _ in range(2 * nb)]
        bs = [dev(torch.randn(64, generator=g) * 0.1) for _ in range(2 * nb + 1)]
        us = [ops.pack_conv3x3_wino(x) for x in ws]
        self.wt = torch.randn(64, 64, 3, 3, generator=g) * 0.05          # (cin, cout, 3, 3)
        self.bt = torch.randn(64, generator=g) * 0.1

        def make(A, B):
            layers = [dict(x=self.lr, x2=self.s2d, u=us[0], bias=bs[0], cin=cin0, act=1, y=A)]
            for b in range(nb):
                layers.append(dict(x=A, u=us[1 + 2 * b], bias=bs[1 + 2 * b], cin=64, act=1, y=B))
                layers.append(dict(x=B, u=us[2 + 2 * b], bias=bs[2 + 2 * b], cin=64, act=0, res=A, y=A))
            return layers
        self.A1, self.B1, self.A2, self.B2 = (torch.empty(1, 64, h, w, device='cuda') for _ in range(4))
        self.seq = make(self.A1, self.B1)
        self.res = ops.WinoResident(make(self.A2, self.B2), 64, h, w)

    def refill(self):
        self.lr.uniform_(-1, 1)
        if self.s2d is not None:
            self.s2d.uniform_(-1, 1)

    def run_seq(self):
        for d in self.seq:
            self.ops.conv3x3_wino(d['x'], d['u'], d['bias'], d['cin'], 64, d['act'], x2=d.get('x2'), res=d.get('res'),
                                  out=d['y'])

    def tail(self):
        return dict(u=self.ops.pack_wres_convt(dev(self.wt)), bias=dev(self.bt),
                    y=torch.empty(1, 64, 2 * self.h, 2 * self.w, device='cuda'), act=1)


def need(ops, h, w):
    if not ops.WinoResident.supported(64, h, w):
        pytest.skip('frame does not fit one block per CU on this device')


@pytest.mark.parametrize('h,w', [(2, 2), (8, 24), (26, 70), (30, 50)])
def test_tail_accuracy(ops, h, w):
    """One live tile (every other lane dead), exactly one full block, partial blocks on the right and at the bottom:
    every output written, and within 3e-6 of the output scale of fp64 conv_transpose2d + ReLU and of ops.convt3x3s2."""
    need(ops, h, w)
    b = Body(ops, h, w, nb=1)
    ct = b.tail()
    pk, _, _, _ = ops.pack_conv3x3(dev(b.wt), transposed=True)
    for it in range(2):
        b.refill()
        ct['y'].fill_(float('nan'))
        b.run_seq()
        ref_gpu = ops.convt3x3s2(b.A1, pk, dev(b.bt), 64, 1)
        b.res.run(convt=ct)
        torch.cuda.synchronize()
        assert b.res.bailouts() == 0
        ref = torch.relu(torch.nn.functional.conv_transpose2d(b.A1.cpu().double(), b.wt.double(), b.bt.double(), 2, 1, 1))
        scale = ref.abs().max().item()
        assert not torch.isnan(ct['y']).any()
        e64 = (ct['y'].cpu().double() - ref).abs().max().item() / scale
        egpu = (ct['y'] - ref_gpu).abs().max().item() / scale
        print('tail %dx%d launch %d: %.3g of the output scale against fp64, %.3g against convt3x3s2 (bound 3e-6)'
              % (h, w, it, e64, egpu))
        assert e64 <= 3e-6, it
        assert egpu <= 3e-6, it


@pytest.mark.parametrize('h,w', [(8, 24), (26, 70)])
def test_tail_is_deterministic_and_leaves_the_body_alone(ops, h, w):
    """Three launches on the same inputs give bit-identical tail outputs, and the launch without the tail still
    writes the body's output equal to the per-layer launches."""
    need(ops, h, w)
    b = Body(ops, h, w, nb=1)
    b.refill()
    b.run_seq()
    outs = []
    for it in range(3):
        ct = b.tail()
        ct['y'].fill_(float('nan'))
        b.res.run(convt=ct)
        torch.cuda.synchronize()
        outs.append(ct['y'])
    assert b.res.bailouts() == 0
    assert not torch.isnan(outs[0]).any()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    b.A2.fill_(float('nan'))
    b.res.run()
    torch.cuda.synchronize()
    assert torch.equal(b.A1, b.A2)


@pytest.mark.parametrize('h,w', [(8, 24), (26, 70)])
@pytest.mark.parametrize('cin0,c1', [(51, 3), (17, 3), (33, 33)])
def test_conv_in_k_steps(ops, h, w, cin0, c1):
    """conv_in runs 2 * ceil(cin / 8) K steps (51 channels: 14 instead of 16; 3 + 14: 6 instead of 8; one source of 33:
    10 instead of 12): the skipped steps added exact zeros, so four consecutive launches still equal the per-layer
    Winograd launches bit for bit."""
    need(ops, h, w)
    b = Body(ops, h, w, nb=1, cin0=cin0, c1=c1, seed=37)
    for it in range(4):
        b.refill()
        b.A2.fill_(float('nan'))
        b.run_seq()
        b.res.run()
        torch.cuda.synchronize()
        assert b.res.bailouts() == 0
        assert torch.equal(b.A1, b.A2), (it, (b.A1 - b.A2).abs().max().item(), int((b.A1 != b.A2).sum()))
