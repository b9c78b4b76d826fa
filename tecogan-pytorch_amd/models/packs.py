"""The packed-weight store: every layout a kernel reads weights in that is not the nn.Parameter itself.

FORMS names each derived form once and gives it one builder.  A builder takes the owner (a _Conv, a _Conv4 or, for the
chained body, the SRNet) and the form's explicit arguments, and reads nothing but the owner's parameters and those
arguments; it returns what the consumer needs, a tensor or the small tuple the pack functions of `ops` return.

get(owner, form, *args) is the one lookup.  The entry's key is (form, *args): whatever a builder reads besides the weights
is in the key.  An entry is valid while the version of every parameter its builder reads is unchanged -- for a layer
ops.param_version(weight), for the body the tuple over its layers.  param_version contains data_ptr(), so a move to
another device is a new version too.  An optimiser step, load_state_dict and .data assignment move it by themselves; a
write through the raw pointer does not, and its writer calls ops.bump_version: the fused Adam (models/optim.py), the
broadcast of the module states (base_model.sync_module_states) and the VGG19 loader (vgg_nets.load_vgg19_state_dict).

The entries live ON the owner object: a process-wide table keyed by id(owner) would hand a new model the stale packs of a
freed one whose id, storage address and version counters it re-uses.  They live as long as the owner.

Next to the store: the one place that chooses a plain 3x3 layer's forward form (conv3x3_forward, prefers_wino).
ops.RowChain and the fp16 packs of the C plan pack plain tensors handed to them and are not layers' forms.
"""
import functools

import torch

from .. import _lib as L
from .. import ops


# space-to-depth embeddings of ConvTranspose2d(k3, s2, p1, op1) (oy = 2*iy - 1 + ky  <=>  ky -> (phase, tap)) and of
# Conv2d(k4, s2, p1) (2*oy - 1 + ky = 2*(oy + ty - 1) + py) into 3x3 / stride-1 weights
_KT = {0: (1, 0), 1: (0, 1), 2: (1, 1)}              # convT: ky -> (py, ty)
_K4 = {0: (1, 0), 1: (0, 1), 2: (1, 1), 3: (0, 2)}   # conv4: ky -> (py, ty)
_IDX = {}


def _embed_index(kind, a, b, device):
    """Flat gather indices of the space-to-depth embeddings, built once per shape:
    `fwd` maps every element of the embedded 3x3 weight to its source element (or to a
    trailing zero slot), `inv` maps every element of the original weight to its slot in the
    embedded tensor.  One index_select then replaces 9 / 16 strided slice copies."""
    key = (kind, a, b, str(device))
    ent = _IDX.get(key)
    if ent is None:
        table = _KT if kind == 'convt' else _K4
        k = len(table)
        src = torch.arange(a * b * k * k, dtype=torch.int64).view(a, b, k, k)
        # convt: (ci, co, 3, 3) -> (ci, 4co, 3, 3); conv4: (co, ci, 4, 4) -> (co, 4ci, 3, 3)
        emb = torch.full((a, 4 * b, 3, 3), a * b * k * k, dtype=torch.int64)
        for ky, (py, ty) in table.items():
            for kx, (px, tx) in table.items():
                ph = py * 2 + px
                emb[:, ph * b:(ph + 1) * b, ty, tx] = src[:, :, ky, kx]
        fwd = emb.reshape(-1)
        inv = torch.empty(a * b * k * k, dtype=torch.int64)
        valid = fwd < a * b * k * k
        inv[fwd[valid]] = torch.nonzero(valid).reshape(-1)
        ent = _IDX[key] = (fwd.to(device), inv.to(device))
    return ent


def _embed(kind, w):
    """convt: (ci, co, 3, 3) -> conv weight (cout_op = ci, cin_op = 4*co, 3, 3) acting on s2d(dY);
    conv4: (co, ci, 4, 4) -> (co, 4*ci, 3, 3) acting on s2d(x, 2)."""
    a, b = w.shape[:2]
    fwd, _ = _embed_index(kind, a, b, w.device)
    return ops.index_gather(w.contiguous(), fwd).view(a, 4 * b, 3, 3)   # out-of-range slot = 0


_convt_embed, _conv4_embed = functools.partial(_embed, 'convt'), functools.partial(_embed, 'conv4')


def _plain(layer):
    return layer.weight.detach().contiguous()


def _direct(layer):
    """(packed, ocb) of the MFMA forward kernel; of a transposed layer, of its sub-pixel phase kernel."""
    pk, _, _, ocb = ops.pack_conv3x3(layer.weight, transposed=layer.transposed)
    return pk, ocb


def body_layers(srnet):
    """conv_in and the residual-block convs, in launch order: the layers of the chained body."""
    out = [srnet.conv_in['0']]
    for rb in srnet.resblocks:
        pair = rb.conv              # (taken once: the body's version walks these on every lookup)
        out += (pair['0'], pair['2'])
    return out


def _body(srnet, layout, c_lr):
    """(layers, forward packs, data-gradient packs) of the body: all 2 x (1 + 2nb) packs in the chained kernels' layout, by
    two launches -- and the layers they are of, so that a hit spares the consumer a second walk over the network."""
    layers = body_layers(srnet)
    ws = [m.weight.detach() for m in layers]
    f = ops.chain_pack([(wt, 0, wt.shape[1], 0) for wt in ws], layout)
    # (the data gradient of conv_in only reaches `tran`: the input channels from c_lr on)
    d = ops.chain_pack([(ws[0], c_lr, ws[0].shape[1] - c_lr, 2)] + [(wt, 0, wt.shape[1], 2) for wt in ws[1:]], layout)
    return layers, f, d


FORMS = {
    # -- _Conv, forward
    'direct': _direct,
    'wino': lambda m: ops.pack_conv3x3_wino(_plain(m)),
    # -- _Conv, data gradient: the rot180 pack onto input channels [lo, hi) (the whole layer, or one source of a two-source
    # one); in Winograd form; the rot180, transposed OIHW taps of the two VALU kernels (onto an image, from a small head)
    'dgrad': lambda m, lo, hi: ops.pack_conv3x3_dgrad(m.weight.detach()[:, lo:hi].contiguous()),
    'dgrad_wino': lambda m: ops.pack_conv3x3_wino(_plain(m), transposed=2),
    'dgrad_small': lambda m: m.weight.detach().flip(2, 3).permute(1, 0, 2, 3).contiguous(),
    'dgrad_fewin': lambda m: m.weight.detach().transpose(0, 1).flip(2, 3).contiguous(),
    # -- transposed _Conv: data gradient as a stride-2 conv of dZ / as a conv3x3 on s2d(dZ); the resident launch's tail
    'convt_dgrad_s2': lambda m: ops.pack_conv3x3(_plain(m), ocb=64)[0],
    'convt_dgrad_embed': lambda m: ops.pack_conv3x3(_convt_embed(m.weight.detach())),
    'wres_convt': lambda m: ops.pack_wres_convt(_plain(m)),
    # -- _Conv4: the direct K = 16 ci pair (forward, data gradient); forward / data gradient embedded on s2d(x)
    'conv4_direct': lambda m: ops.pack_conv4x4s2(_plain(m)),
    'conv4_embed': lambda m: ops.pack_conv3x3(_conv4_embed(m.weight.detach())),
    'conv4_dgrad_embed': lambda m: ops.pack_conv3x3_dgrad(_conv4_embed(m.weight.detach())),
    # -- SRNet: the chained body; args (layout, c_lr)
    'body': _body,
}


def get(owner, form, *args):
    """The form `form` of `owner`'s weights, built on first use and again after any weight its builder reads changed:
    the layer's own; for the body every layer's (a partial load / freeze must re-pack too)."""
    ver = ops.param_version(owner.weight) if form != 'body' else \
        tuple(ops.param_version(m.weight) for m in body_layers(owner))
    key = (form,) + args
    try:
        ent = owner.__dict__['_packs'][key]
        if ent[0] == ver:
            return ent[1]
    except KeyError:
        pass
    value = FORMS[form](owner, *args)
    owner.__dict__.setdefault('_packs', {})[key] = (ver, value)
    return value


def held(owner):
    """{(form, *args): (version, value)} of what `owner` holds now (tests, accounting)."""
    return owner.__dict__.get('_packs', {})


_WINO_RULE = {}


def prefers_wino(n, cin, cout, h, w):
    """tg_conv3x3_prefers_wino, memoised per shape (the tape asks ~2000 times per training step).
    (`cout % 64` here; packed_wino() and the C plan also admit cout == 32 -- a difference that is known and kept.)"""
    if cout % 64 or cin < 16:
        return False
    key = (n, cin, cout, h, w)
    r = _WINO_RULE.get(key)
    if r is None:
        r = _WINO_RULE[key] = bool(L.lib().tg_conv3x3_prefers_wino(n, cin, cout, h, w))
    return r


def conv3x3_forward(layer, x, act=ops.ACT_NONE, x2=None, res=None, out=None, pool=False):
    """One 3x3 layer forward, inference and the tape alike: the Winograd form when the rule prefers it for this shape
    and the layer has that pack, else the sub-pixel phase kernel of a transposed layer / the MFMA kernel (with `pool`
    folded in).  A holder without packed_wino (tests) has no Winograd form."""
    cin, cout = layer.cin, layer.cout
    if getattr(layer, 'transposed', False):
        return ops.convt3x3s2(x, layer.packed()[0], layer.bias, cout, act, out=out)
    if not pool and hasattr(layer, 'packed_wino') and prefers_wino(x.shape[0], cin, cout, x.shape[2], x.shape[3]):
        u = layer.packed_wino()
        if u is not None:
            return ops.conv3x3_wino(x, u, layer.bias, cin, cout, act, x2=x2, res=res, out=out)
    pk, ocb = layer.packed()
    return ops.conv3x3(x, pk, layer.bias, cin, cout, ocb, act, x2=x2, res=res, out=out, pool=pool)
