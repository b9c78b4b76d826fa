"""The resident SRNet launch's hand-over with the per-workgroup ring table (tg_conv3x3_wino_res.hip): every boundary
thread decodes its ring items from a table the launch fills once, instead of deriving them in each of its hand-overs.

conv_in (3 + 48 channels) + two residual blocks = five layers, four hand-overs (five with the tail): both parities of
the exchange buffer, both layer kinds.  Shapes: one block (nothing to fetch), 2 x 2 full blocks, a centre block with
all eight neighbours, 2 x 2 blocks with two live rows / columns, and partial blocks on both edges.  The body must
equal the per-layer Winograd launches bit for bit; the transposed-conv tail is held to the bound of
tests/test_hip_wres_ct_wino.py (3e-6 of the output scale against fp64 and against tg_convt3x3s2_fwd).  Three launches
in a row on refilled inputs: the tag base advances and the table is rebuilt by each launch."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(8, 24), (16, 48), (24, 72), (10, 26), (26, 70)]
NB = 2
TAIL_BOUND = 3e-6           # of the output scale: tests/test_hip_wres_ct_wino.py


@pytest.fixture(scope='module')
def ops():
    import tecogan_pytorch_amd.ops as ops_
    from tecogan_pytorch_amd import _lib
    _lib.lib()
    return ops_


def dev(x):
    return x.cuda().contiguous()


class Body:
    """The per-layer launches into (A1, B1) and the resident launch into (A2, B2), as tests/test_hip_wres_ct_wino.py."""

    def __init__(self, ops, h, w, seed=41):
        g = torch.Generator().manual_seed(seed)
        self.ops, self.h, self.w = ops, h, w
        self.lr = dev(torch.rand(1, 3, h, w, generator=g))
        self.s2d = dev(torch.rand(1, 48, h, w, generator=g))
        ws = [dev(torch.randn(64, 51, 3, 3, generator=g) * 0.04)] + \
             [dev(torch.randn(64, 64, 3, 3, generator=g) * 0.03) for _ in range(2 * NB)]
        bs = [dev(torch.randn(64, generator=g) * 0.1) for _ in range(2 * NB + 1)]
        us = [ops.pack_conv3x3_wino(x) for x in ws]
        self.wt = torch.randn(64, 64, 3, 3, generator=g) * 0.05          # (cin, cout, 3, 3)
        self.bt = torch.randn(64, generator=g) * 0.1

        def make(A, B):
            layers = [dict(x=self.lr, x2=self.s2d, u=us[0], bias=bs[0], cin=51, act=1, y=A)]
            for b in range(NB):
                layers.append(dict(x=A, u=us[1 + 2 * b], bias=bs[1 + 2 * b], cin=64, act=1, y=B))
                layers.append(dict(x=B, u=us[2 + 2 * b], bias=bs[2 + 2 * b], cin=64, act=0, res=A, y=A))
            return layers
        self.A1, self.B1, self.A2, self.B2 = (torch.empty(1, 64, h, w, device='cuda') for _ in range(4))
        self.seq = make(self.A1, self.B1)
        self.res = ops.WinoResident(make(self.A2, self.B2), 64, h, w)

    def refill(self):
        self.lr.uniform_(-1, 1)
        self.s2d.uniform_(-1, 1)

    def run_seq(self):
        for d in self.seq:
            self.ops.conv3x3_wino(d['x'], d['u'], d['bias'], d['cin'], 64, d['act'], x2=d.get('x2'), res=d.get('res'),
                                  out=d['y'])


def need(ops, h, w):
    """Every shape here is at most nine blocks: on the MI355X (256 CUs) the launch must take them; other devices may skip."""
    ok = ops.WinoResident.supported(64, h, w)
    if torch.cuda.get_device_properties(0).multi_processor_count >= 256:
        assert ok, 'the resident launch refuses %dx%d on a 256-CU part' % (h, w)
    elif not ok:
        pytest.skip('frame does not fit one block per CU on this device')


@pytest.mark.parametrize('h,w', SHAPES)
def test_body_equals_the_per_layer_launches(ops, h, w):
    need(ops, h, w)
    b = Body(ops, h, w)
    for it in range(3):
        b.refill()
        b.A2.fill_(float('nan'))
        b.run_seq()
        b.res.run()
        torch.cuda.synchronize()
        assert b.res.bailouts() == 0, it
        assert torch.equal(b.A1, b.A2), (it, (b.A1 - b.A2).abs().max().item(), int((b.A1 != b.A2).sum()))


@pytest.mark.parametrize('h,w', SHAPES)
def test_tail_behind_the_last_hand_over(ops, h, w):
    """With the transposed-conv tail the last layer hands over like any other (its ring feeds the tail's windows): the
    tail's output within the parent's bound of fp64 conv_transpose2d + ReLU of the per-layer body and of ops.convt3x3s2,
    every output written, and the same bits from a second launch on the same inputs."""
    need(ops, h, w)
    b = Body(ops, h, w)
    ct = dict(u=ops.pack_wres_convt(dev(b.wt)), bias=dev(b.bt), y=torch.empty(1, 64, 2 * h, 2 * w, device='cuda'), act=1)
    pk, _, _, _ = ops.pack_conv3x3(dev(b.wt), transposed=True)
    for it in range(3):
        b.refill()
        ct['y'].fill_(float('nan'))
        b.run_seq()
        ref_gpu = ops.convt3x3s2(b.A1, pk, dev(b.bt), 64, 1)
        b.res.run(convt=ct)
        torch.cuda.synchronize()
        assert b.res.bailouts() == 0, it
        first = ct['y'].clone()
        ref = torch.relu(torch.nn.functional.conv_transpose2d(b.A1.cpu().double(), b.wt.double(), b.bt.double(), 2, 1, 1))
        scale = ref.abs().max().item()
        assert not torch.isnan(first).any(), it
        e64 = (first.cpu().double() - ref).abs().max().item() / scale
        egpu = (first - ref_gpu).abs().max().item() / scale
        print('tail %dx%d launch %d: %.3g of the output scale against fp64, %.3g against convt3x3s2 (bound %g)'
              % (h, w, it, e64, egpu, TAIL_BOUND))
        assert e64 <= TAIL_BOUND, it
        assert egpu <= TAIL_BOUND, it
        ct['y'].fill_(float('nan'))
        b.res.run(convt=ct)
        torch.cuda.synchronize()
        assert b.res.bailouts() == 0, it
        assert torch.equal(first, ct['y']), it
