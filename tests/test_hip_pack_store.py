"""The packed-weight store (models/packs.py) on the GPU: every form of the table follows every way a weight can change.
A form taken again after the change equals, element for element, the same form of a FRESH layer that was loaded with the
updated weights -- a stale pack gives no error and no NaN, only last step's weights.  Only pack kernels are launched,
except by the last test: one inference frame before and after an in-place update of every parameter."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _nets():
    from tecogan_pytorch_amd.models.networks import tecogan_nets
    return tecogan_nets


def _named(name, make):
    make.__name__ = name
    return make


def conv(ci, co, transposed=False):
    return _named(f'conv{ci}x{co}' + ('T' if transposed else ''), lambda: _nets()._Conv(ci, co, transposed=transposed))


def conv4(ci, co):
    return _named(f'conv4_{ci}x{co}', lambda: _nets()._Conv4(ci, co))


def srnet():
    return _nets().SRNet(3, 3, 64, 1, None, 4)


# (what makes the owner, form, its arguments): the smallest layers that reach every builder
CASES = [(conv(ci, 64), form, args) for ci in (16, 64)
         for form, args in (('direct', ()), ('wino', ()), ('dgrad', (0, ci)), ('dgrad_wino', ()))]
CASES += [(conv(51, 64), 'dgrad', (0, 3)), (conv(51, 64), 'dgrad', (3, 51))]             # conv_in's two sources
CASES += [(conv(64, 3), 'dgrad_fewin', ()), (conv(64, 3), 'dgrad', (0, 64)), (conv(64, 3), 'direct', ()),   # the head
          (conv(3, 64), 'dgrad_small', ())]                                                # onto an image
CASES += [(conv(64, 64, transposed=True), form, ())
          for form in ('direct', 'convt_dgrad_s2', 'convt_dgrad_embed', 'wres_convt')]
CASES += [(conv4(64, 64), form, ()) for form in ('conv4_direct', 'conv4_embed', 'conv4_dgrad_embed')]
CASES += [(srnet, 'body', None)]             # (layout, c_lr): what _ChainState.parts(1, 16, 16) names, below


def _case_id(c):
    make, form, args = c
    return f'{form}{list(args) if args else ""}-{make.__name__}'


# -- the sources of a weight change: each leaves the weights scaled by 1.01 ------------------------------------------
def in_place(owner, target):
    with torch.no_grad():
        target.weight.mul_(1.01)


def raw_pointer_writer(owner, target):
    from tecogan_pytorch_amd import ops
    w = target.weight
    before = ops.param_version(w)
    w.data.mul_(1.01)                        # .data has a version counter of its own: the write is invisible, as the
    assert ops.param_version(w) == before    # fused Adam's through the raw pointer is
    ops.bump_version(w)


def load_state_dict(owner, target):
    sd = {k: v.clone() for k, v in owner.state_dict().items()}
    key = next(k for k, v in owner.state_dict(keep_vars=True).items() if v is target.weight)
    sd[key] = sd[key] * 1.01
    owner.load_state_dict(sd, strict=True)


def new_storage(owner, target):
    target.weight.data = target.weight.data * 1.01


CHANGES = [in_place, raw_pointer_writer, load_state_dict, new_storage]


def same(a, b):
    if isinstance(a, torch.nn.Module):           # (the body's entry names its layers: the fresh network's are its own)
        return type(a) is type(b)
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.shape == b.shape and torch.equal(a, b)
    if isinstance(a, (tuple, list)):
        return isinstance(b, (tuple, list)) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return a == b


def identical(a, b):
    """The same objects, not equal ones."""
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(identical(x, y) for x, y in zip(a, b))
    return a is b if torch.is_tensor(a) else a == b


@pytest.mark.parametrize('change', CHANGES, ids=lambda f: f.__name__)
@pytest.mark.parametrize('case', CASES, ids=_case_id)
def test_every_form_follows_every_weight_change(case, change):
    from tecogan_pytorch_amd.models import packs
    from tecogan_pytorch_amd.models.train_chain import _ChainState
    make, form, args = case
    assert form in packs.FORMS
    torch.manual_seed(7)
    owner = make().cuda()
    target = owner
    if form == 'body':
        parts = _ChainState.parts(1, 16, 16)
        if parts == 0:
            pytest.skip('no chained launch for (1, 16, 16) on this device')
        args = (16 if parts == 4 else 64, 3)
        target = packs.body_layers(owner)[-1]                 # not the first layer: every layer is part of the version
    old = packs.get(owner, form, *args)
    assert identical(packs.get(owner, form, *args), old)
    w0 = target.weight.detach().clone()
    change(owner, target)
    assert torch.equal(target.weight.detach(), w0 * 1.01)
    new = packs.get(owner, form, *args)
    assert identical(packs.get(owner, form, *args), new)
    fresh = make().cuda()
    fresh.load_state_dict(owner.state_dict(), strict=True)
    assert packs.held(fresh) == {}
    want = packs.get(fresh, form, *args)
    torch.cuda.synchronize()
    assert same(new, want), 'the form taken after the change is not the form of the updated weights'
    assert not same(old, want), 'the change did not reach the form: the case checks nothing'


def test_every_form_of_the_table_has_a_case():
    from tecogan_pytorch_amd.models import packs
    assert {form for _, form, _ in CASES} == set(packs.FORMS)


def test_inference_follows_an_in_place_update_of_every_parameter():
    """FRNet.step builds its plan from the layers' forms (direct, Winograd, the resident launch's tail): after an update
    the frame is that of a fresh network with the updated weights, bit for bit, and not the one before."""
    FRNet = _nets().FRNet
    torch.manual_seed(11)
    net = FRNet(3, 3, 64, 1, 'BD', 4).cuda().eval()
    g = torch.Generator().manual_seed(5)
    lr, lr_prev, hr_prev = (torch.rand(1, 3, s, s, generator=g).cuda() for s in (16, 16, 64))
    with torch.no_grad():
        first = net.step(lr, lr_prev, hr_prev).clone()
        for p in net.parameters():
            p.mul_(1.01)
        second = net.step(lr, lr_prev, hr_prev).clone()
        fresh = FRNet(3, 3, 64, 1, 'BD', 4)
        fresh.load_state_dict(net.state_dict(), strict=True)
        want = fresh.cuda().eval().step(lr, lr_prev, hr_prev).clone()
    torch.cuda.synchronize()
    assert first.shape == want.shape == (1, 3, 64, 64) and bool(torch.isfinite(want).all())
    assert torch.equal(second, want)
    assert not torch.equal(first, want)
