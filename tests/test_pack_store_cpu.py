"""The packed-weight store (models/packs.py) without a GPU and without the library: CPU parameters, and counting stubs in
place of the builders.  What is checked is the store's bookkeeping -- when a form is built again, what its key holds, who
owns an entry -- and, by reading the sources, that the store is the only holder of derived weight forms."""
import gc
import glob
import os
import re
import weakref

import pytest
import torch

import tecogan_pytorch_amd  # noqa: F401
from tecogan_pytorch_amd import ops
from tecogan_pytorch_amd.models import packs
from tecogan_pytorch_amd.models.networks.tecogan_nets import SRNet, _Conv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'tecogan-pytorch_amd')
STORE = os.path.join('models', 'packs.py')


class Built:
    """What a stub returns: a fresh object per build (weak-referenceable), with the arguments it was built from."""

    def __init__(self, form, args):
        self.form, self.args = form, args


@pytest.fixture
def counts(monkeypatch):
    """Every builder of the table replaced by a stub that counts its calls per (form, *args)."""
    n = {}
    for name in packs.FORMS:
        def stub(owner, *args, _name=name):
            n[(_name,) + args] = n.get((_name,) + args, 0) + 1
            return Built(_name, args)
        monkeypatch.setitem(packs.FORMS, name, stub)
    return n


# -- the sources of a weight change ---------------------------------------------------------------------------------
def _in_place(layer):
    with torch.no_grad():
        layer.weight.mul_(1.01)


def _raw_pointer_writer(layer):
    ops.bump_version(layer.weight)          # what the fused Adam, the broadcast and the VGG loader do after their write


def _load_state_dict(layer):
    layer.load_state_dict({k: v * 1.01 for k, v in layer.state_dict().items()})


def _new_storage(layer):
    layer.weight.data = layer.weight.data * 1.01


CHANGES = [_in_place, _raw_pointer_writer, _load_state_dict, _new_storage]


@pytest.mark.parametrize('change', CHANGES, ids=lambda f: f.__name__.strip('_'))
def test_a_form_is_built_once_per_weight_version(counts, change):
    layer = _Conv(4, 8)
    a = packs.get(layer, 'direct')
    assert packs.get(layer, 'direct') is a and packs.get(layer, 'direct') is a and counts == {('direct',): 1}
    old = ops.param_version(layer.weight)
    change(layer)
    assert ops.param_version(layer.weight) != old
    b = packs.get(layer, 'direct')
    assert b is not a and counts == {('direct',): 2}
    assert packs.get(layer, 'direct') is b and counts == {('direct',): 2}
    # a change of the bias is not a change of anything a layer's builder reads
    with torch.no_grad():
        layer.bias.add_(1.0)
    assert packs.get(layer, 'direct') is b and counts == {('direct',): 2}


def test_the_arguments_are_part_of_the_key(counts):
    layer = _Conv(8, 4)
    a3, a5 = packs.get(layer, 'dgrad', 0, 3), packs.get(layer, 'dgrad', 0, 5)
    b3, b5 = packs.get(layer, 'dgrad', 3, 8), packs.get(layer, 'dgrad', 5, 8)
    assert (a3.args, a5.args, b3.args, b5.args) == ((0, 3), (0, 5), (3, 8), (5, 8))
    # neither evicts the other: all four are still there, and none is built again
    assert packs.get(layer, 'dgrad', 0, 3) is a3 and packs.get(layer, 'dgrad', 0, 5) is a5
    assert packs.get(layer, 'dgrad', 3, 8) is b3 and packs.get(layer, 'dgrad', 5, 8) is b5
    assert counts == {('dgrad', 0, 3): 1, ('dgrad', 0, 5): 1, ('dgrad', 3, 8): 1, ('dgrad', 5, 8): 1}
    assert set(packs.held(layer)) == set(counts)
    # a new weight version makes every one of them stale, each on its own
    _in_place(layer)
    assert packs.get(layer, 'dgrad', 0, 5) is not a5 and packs.get(layer, 'dgrad', 0, 3) is not a3
    assert counts[('dgrad', 0, 3)] == 2 and counts[('dgrad', 0, 5)] == 2 and counts[('dgrad', 3, 8)] == 1


def test_two_forms_of_one_layer_never_share_an_entry(counts):
    layer = _Conv(16, 64)
    got = {name: packs.get(layer, name) for name in packs.FORMS if name not in ('dgrad', 'body')}
    got['dgrad'] = packs.get(layer, 'dgrad', 0, 16)
    assert len({id(v) for v in got.values()}) == len(got) and all(v.form == name for name, v in got.items())
    assert all(c == 1 for c in counts.values()) and len(counts) == len(got) == len(packs.held(layer))
    for name, v in got.items():
        assert packs.get(layer, *((name,) if name != 'dgrad' else (name, 0, 16))) is v
    with pytest.raises(KeyError):
        packs.get(layer, 'no such form')


def test_layers_do_not_see_each_others_entries(counts):
    a, b = _Conv(4, 8), _Conv(4, 8)
    with torch.no_grad():
        b.weight.copy_(a.weight)            # equal values, equal version counters: still two owners
    pa = packs.get(a, 'direct')
    assert packs.held(b) == {}
    pb = packs.get(b, 'direct')
    assert pa is not pb and counts == {('direct',): 2}
    _in_place(a)
    assert packs.get(b, 'direct') is pb and packs.get(a, 'direct') is not pa


def test_entries_live_on_the_owner_and_die_with_it(counts):
    layer = _Conv(4, 8)
    value = packs.get(layer, 'direct')
    assert any(ent[1] is value for store in vars(layer).values() if isinstance(store, dict) for ent in store.values()
               if isinstance(ent, tuple)), 'the entry is not on the layer object'
    gone, was = weakref.ref(value), id(layer)
    del layer, value
    gc.collect()
    assert gone() is None, 'something besides the layer holds the entry'
    # a new layer -- at the freed one's address if the allocator hands it out again -- starts with nothing
    reused = False
    for _ in range(64):
        fresh = _Conv(4, 8)
        assert packs.held(fresh) == {}
        reused = reused or id(fresh) == was
        before = counts[('direct',)]
        packs.get(fresh, 'direct')
        assert counts[('direct',)] == before + 1
        if reused:
            break
        del fresh
    # (no table outside the owners: the module holds no dict keyed by an owner or its id)
    for name, obj in vars(packs).items():
        if isinstance(obj, dict) and name not in ('FORMS', '_KT', '_K4', '_IDX', '_WINO_RULE') and not name.startswith('__'):
            raise AssertionError(f'packs.{name}: a module-level dict')


def test_the_body_follows_every_one_of_its_layers(counts):
    net = SRNet(3, 3, 8, 2, None, 4)
    layers = packs.body_layers(net)
    assert len(layers) == 5 and layers[0] is net.conv_in['0'] and layers[-1] is net.resblocks[1].conv['2']
    cur = packs.get(net, 'body', 64, 3)
    assert packs.get(net, 'body', 64, 3) is cur and counts == {('body', 64, 3): 1}
    for i, m in enumerate(layers):
        for change in CHANGES:
            change(m)
            new = packs.get(net, 'body', 64, 3)
            assert new is not cur, f'layer {i}, {change.__name__}: the stale body packs were handed out'
            assert packs.get(net, 'body', 64, 3) is new
            cur = new
    assert counts == {('body', 64, 3): 1 + len(layers) * len(CHANGES)}
    # the layout and the input split are arguments, and so other entries
    assert packs.get(net, 'body', 16, 3) is not cur and packs.get(net, 'body', 64, 3) is cur
    # a layer outside the body (an up-sampling layer, the head) is not read by its builder
    _in_place(net.conv_out)
    _in_place(net.conv_up['0'])
    assert packs.get(net, 'body', 64, 3) is cur


def test_layer_methods_go_through_the_store(counts):
    layer = _Conv(16, 64)
    pk = layer.packed()
    assert isinstance(pk, Built) and pk.form == 'direct' and layer.packed() is pk
    u = layer.packed_wino()
    assert u.form == 'wino' and layer.packed_wino() is u
    # no Winograd form: transposed, cout neither 32 nor a multiple of 64, cin < 16 -- and nothing is built for them
    for m in (_Conv(16, 64, transposed=True), _Conv(16, 48), _Conv(8, 64)):
        assert m.packed_wino() is None and packs.held(m) == {}
    assert _Conv(16, 32).packed_wino().form == 'wino'
    assert counts == {('direct',): 1, ('wino',): 2}


# -- the sources ----------------------------------------------------------------------------------------------------
FORBIDDEN = {
    'the old per-owner dict': re.compile(r'_tg_pack_cache'),
    'the old cache class / instance': re.compile(r'\bConvCache\b|\b_CACHE\b'),
    'a cache slot assigned on a layer': re.compile(r'\.\s*_cache(?:_u)?\s*=(?!=)'),
    'the second version helper': re.compile(r'\bdef\s+_ver\b|\b_ver\s*\('),
}
DIRECT_PACK = re.compile(r'\bops\s*\.\s*(?:pack_\w+|chain_pack)\s*\(')


def _sources():
    files = sorted(glob.glob(os.path.join(PKG, '**', '*.py'), recursive=True))
    return {os.path.relpath(f, PKG): open(f).read() for f in files}


def test_only_the_store_holds_derived_weight_forms():
    src = _sources()
    assert len(src) >= 20 and STORE in src
    hits = sorted((name, what) for name, text in src.items() if name != STORE
                  for what, rx in FORBIDDEN.items() if rx.search(text))
    assert not hits, f'outside {STORE}: {hits} -- a derived weight form is a FORMS entry, taken with packs.get'
    tape = src[os.path.join('models', 'train_graph.py')]
    assert not DIRECT_PACK.search(tape), 'train_graph.py packs weights itself: packing goes through packs.FORMS'
    assert 'packs.get(' in tape
    # one version vocabulary, defined in one place
    defs = [(name, m.group(1)) for name, text in src.items()
            for m in re.finditer(r'^def (param_version|bump_version)\b', text, re.M)]
    assert sorted(defs) == [('ops.py', 'bump_version'), ('ops.py', 'param_version')]


def test_the_patterns_catch_what_they_are_for():
    bad = {'the old per-owner dict': "store = owner.__dict__.setdefault('_tg_pack_cache', {})",
           'the old cache class / instance': "wk = _CACHE.get(layer, ('ctd',), _ver(w), lambda: 0)",
           'a cache slot assigned on a layer': '        self._cache_u = (key, u)',
           'the second version helper': 'def _ver(w):'}
    for what, line in bad.items():
        assert FORBIDDEN[what].search(line), line
    assert FORBIDDEN['a cache slot assigned on a layer'].search('self._cache = None')
    assert FORBIDDEN['the old cache class / instance'].search('class ConvCache:')
    good = ['torch.cuda.empty_cache()', "os.environ.get('XDG_CACHE_HOME')", '@functools.lru_cache(maxsize=None)',
            'if self._cache == key:', 'key = self._plan_cache_key(n, h, w)', 'wk = self._weights_key()']
    for line in good:
        assert not any(rx.search(line) for rx in FORBIDDEN.values()), line
    assert DIRECT_PACK.search('pkd = ops.pack_conv3x3_dgrad(w)') and DIRECT_PACK.search('f = ops.chain_pack(items, 64)')
    assert not DIRECT_PACK.search("pkd = packs.get(layer, 'dgrad', 0, c1)")
