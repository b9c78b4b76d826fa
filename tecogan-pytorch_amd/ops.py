"""Tensor-level wrappers over the C ABI.  PyTorch is plumbing here: it owns the
device memory and the stream; every computation is a HIP kernel from
libtecogan_hip.so.  All tensors must be CUDA(HIP) fp32 and contiguous.

This module is the one place where a Python object becomes a raw device address: every entry
point that takes a stream is reached through _call, and every tensor whose address goes in has passed _chk,
_chk_batched or _chk_u8 with the dtype of its prototype before the wrapper allocates or launches anything."""
import ctypes
import math

import numpy as np
import torch

from . import _lib as L
from ._lib import (ACT_NONE, ACT_RELU, ACT_LRELU02, ACT_TANH24,  # noqa: F401
                   UP_NONE, UP_BICUBIC, UP_BILINEAR)

UP_MODE = {'BD': UP_BICUBIC, 'BI': UP_BILINEAR}


_RAW_STREAM = getattr(torch._C, '_cuda_getCurrentRawStream', None)


def _stream():
    """hipStream_t of torch's current stream (the raw-handle query is ~10x cheaper than building a
    torch.cuda.Stream object; a training step asks ~650 times)."""
    if _RAW_STREAM is not None:
        return _RAW_STREAM(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def _call(name, *args):
    """The one way to an entry point that takes a stream: `name`(*args, the current stream), its status checked under
    that same name.  Host-only queries (sizes, picks, *_supported) are plain L.lib() calls."""
    L.check(getattr(L.lib(), name)(*args, _stream()), name)


def _chk(t, name, dtype=torch.float32):
    if not (torch.is_tensor(t) and t.is_cuda):
        raise L.TecoganHipError(f'{name}: expected a CUDA/HIP tensor (no CPU path exists)')
    if t.dtype != dtype:
        raise L.TecoganHipError(f'{name}: expected {dtype}, got {t.dtype}')
    if not t.is_contiguous():
        raise L.TecoganHipError(f'{name}: tensor must be contiguous')
    return t


def _chk_all(dtype=torch.float32, **operands):
    """_chk of every operand, under its keyword as the name."""
    for name, t in operands.items():
        _chk(t, name, dtype)


def _chk_opt(dtype=torch.float32, **operands):
    """_chk_all for optional operands: None (not given) passes."""
    for name, t in operands.items():
        if t is not None:
            _chk(t, name, dtype)


def _chk_list(tensors, name, dtype=torch.float32):
    """_chk of every tensor of a list whose addresses go to the library as one pointer array (_ptr_array)."""
    for t in tensors:
        _chk(t, name, dtype)


def _chk_batched(t, name, dtype=torch.float32, device=True):
    """_chk for an operand whose entry point takes a batch stride (the one-launch bodies): dtype and device as _chk,
    the dimensions behind the batch dimension contiguous, the batch stride free (at least one image)."""
    if not torch.is_tensor(t):
        raise L.TecoganHipError(f'{name}: expected a tensor')
    if t.dtype != dtype:
        raise L.TecoganHipError(f'{name}: expected {dtype}, got {t.dtype}')
    if t.dim() < 2 or not t[0].is_contiguous() or (t.shape[0] > 1 and t.stride(0) < t[0].numel()):
        raise L.TecoganHipError(f'{name}: the dimensions behind the batch dimension must be contiguous and the images '
                                f'apart (shape {tuple(t.shape)}, strides {tuple(t.stride())})')
    if device and not t.is_cuda:
        raise L.TecoganHipError(f'{name}: expected a CUDA/HIP tensor (no CPU path exists)')
    return t


def _chk_u8(t, name):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()):
        raise L.TecoganHipError(f'{name}: expected a contiguous CUDA uint8 tensor, got '
                                + (f'{t.dtype} {t.device} contiguous={t.is_contiguous()}' if torch.is_tensor(t)
                                   else repr(type(t))))
    return t


def _chk_layers(layers, who, packed):
    """Every tensor of the layer dicts of RowChain / WinoChain / WinoResident: activations through _chk_batched (dtype
    and layout of all of them first, then the device), packed weights (`packed`: their key) and biases through _chk."""
    acts = [(f'{who}: layer {i}: {k}', d[k]) for i, d in enumerate(layers) for k in ('x', 'x2', 'res', 'mask', 'y')
            if d.get(k) is not None]
    for name, t in acts:
        _chk_batched(t, name, device=False)
    for name, t in acts:
        _chk_batched(t, name)
    for i, d in enumerate(layers):
        _chk(d[packed], f'{who}: layer {i}: {packed}')
        if d.get('bias') is not None:
            _chk(d['bias'], f'{who}: layer {i}: bias')


def _ptr(t):
    return None if t is None else t.data_ptr()


def _out(out, shape, like, who, dtype=torch.float32, name='out', chk=_chk):
    """The tensor a wrapper writes: a new one of this shape and dtype on `like`'s device, or the given one after the check
    (`chk`) that it is exactly that."""
    if out is None:
        return torch.empty(tuple(shape), dtype=dtype, device=like.device)
    if tuple(chk(out, name, dtype).shape) != tuple(shape) or out.device != like.device:
        raise L.TecoganHipError(f'{who}: {name} is {dtype} {tuple(shape)} on {like.device}, got {tuple(out.shape)} on '
                                f'{out.device}')
    return out


_WORKSPACES = {}


def _workspace(nbytes, device, cached=False):
    """Workspace bytes as the library states them -> a uint8 tensor of that size rounded up to whole 8-byte words (its
    numel() is the size to pass on).  cached: the scratch of the weight-gradient launches, kept and grown per (device,
    stream) -- two models may run their training steps on two streams at the same time."""
    nbytes = (int(nbytes) + 7) // 8 * 8
    if not cached:
        return torch.empty(nbytes, dtype=torch.uint8, device=device)
    key = (str(device), _stream())
    ws = _WORKSPACES.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = _WORKSPACES[key] = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return ws


def param_version(w):
    """Cache key for anything derived from a parameter (packed weights, plans)."""
    return (w.data_ptr(), w._version, getattr(w, '_tg_version', 0))


def bump_version(w):
    """Call after modifying a parameter through its raw pointer (fused Adam)."""
    w._tg_version = getattr(w, '_tg_version', 0) + 1


def pick_ocb(cout):
    return L.lib().tg_conv3x3_pick_ocb(int(cout))


def pack_conv3x3(weight, transposed=False, ocb=None):
    """nn.Conv2d.weight (cout,cin,3,3) [or ConvTranspose2d (cin,cout,3,3)] ->
    kernel layout.  Returns (packed, cin, cout, ocb)."""
    w = _chk(weight, 'weight').detach()
    if w.dim() != 4 or w.shape[2:] != (3, 3):
        raise L.TecoganHipError(f'pack_conv3x3: weight shape {tuple(w.shape)}')
    if transposed:
        cin, cout = w.shape[0], w.shape[1]
        ocb = 64
    else:
        cout, cin = w.shape[0], w.shape[1]
        ocb = ocb or pick_ocb(cout)
    nfl = L.lib().tg_conv3x3_packed_floats(cin, cout, ocb)
    out = torch.empty(nfl, dtype=torch.float32, device=w.device)
    _call('tg_conv3x3_pack', w.data_ptr(), out.data_ptr(), cin, cout, ocb, 1 if transposed else 0)
    return out, cin, cout, ocb


def conv3x3(x, wpk, bias, cin, cout, ocb, act=ACT_NONE, x2=None, res=None, out=None,
            pool=False, ksplit=None, relu_mask=None):
    """y = act(conv3x3(cat[x, x2]) + bias) (+ res) [-> maxpool2 when pool].
    x: (n,c1,h,w), x2: (n,cin-c1,h,w).  Small, deep layers go through the
    deterministic split-K path (ksplit=None: library heuristic).
    relu_mask (shape of y): y is zeroed where relu_mask <= 0 in the same epilogue (the
    ReLU backward of the layer that produced relu_mask)."""
    _chk_all(x=x, wpk=wpk)
    _chk_opt(bias=bias, x2=x2, res=res, relu_mask=relu_mask)
    n, c1, h, w = x.shape
    if ksplit is None:
        ksplit = 1 if (res is not None or relu_mask is not None) else \
            L.lib().tg_conv3x3_pick_ksplit(n, cin, cout, h, w)
    if ksplit > 1:
        if res is not None or relu_mask is not None:
            raise L.TecoganHipError('conv3x3: split-K path has no residual / mask epilogue')
        out = _out(out, (n, cout, h // 2, w // 2) if pool else (n, cout, h, w), x, 'conv3x3')
        part = torch.empty(ksplit * n * cout * h * w, dtype=torch.float32, device=x.device)
        _call('tg_conv3x3_splitk_fwd', x.data_ptr(), c1 * h * w, c1, _ptr(x2), 0 if x2 is None else x2.shape[1] * h * w,
              wpk.data_ptr(), ocb, _ptr(bias), out.data_ptr(), n, cin, cout, h, w, act, ksplit, part.data_ptr(),
              1 if pool else 0)
        return out
    if pool:
        return maxpool2(conv3x3(x, wpk, bias, cin, cout, ocb, act, x2=x2, res=res, ksplit=1))
    if x2 is not None:
        if x2.shape[0] != n or x2.shape[2:] != x.shape[2:] or c1 + x2.shape[1] != cin:
            raise L.TecoganHipError(f'conv3x3: x {tuple(x.shape)} x2 {tuple(x2.shape)} cin {cin}')
    elif c1 != cin:
        raise L.TecoganHipError(f'conv3x3: x has {c1} channels, weights expect {cin}')
    out = _out(out, (n, cout, h, w), x, 'conv3x3')
    if res is not None and res.shape != out.shape:
        raise L.TecoganHipError('conv3x3: residual shape mismatch')
    hw = h * w
    lead = (x.data_ptr(), c1 * hw, c1, _ptr(x2), 0 if x2 is None else x2.shape[1] * hw, wpk.data_ptr(), ocb, _ptr(bias),
            _ptr(res), cout * hw)
    tail = (out.data_ptr(), cout * hw, n, cin, cout, h, w, act)
    if relu_mask is not None:
        if relu_mask.shape != out.shape:
            raise L.TecoganHipError('conv3x3: relu_mask shape mismatch')
        _call('tg_conv3x3_fwd_masked', *lead, relu_mask.data_ptr(), cout * hw, *tail)
    else:
        _call('tg_conv3x3_fwd', *lead, *tail)
    return out


TAPS_ALL, TAPS_01, TAPS_12, TAPS_1 = 0, 1, 2, 3


def conv3x3_phased(x, wpk, cin, cout, ocb, tapsel, cphase, taps_phase0, taps_phase1, out=None, relu_mask=None):
    """conv3x3 (no bias / activation) of a space-to-depth embedded strided conv, skipping the
    taps a sub-pixel phase does not own (include/tecogan_hip.h: tg_conv3x3_fwd_phased)."""
    _chk_all(x=x, wpk=wpk)
    _chk_opt(relu_mask=relu_mask)
    n, c1, h, w = x.shape
    if c1 != cin:
        raise L.TecoganHipError(f'conv3x3_phased: x has {c1} channels, weights expect {cin}')
    out = _out(out, (n, cout, h, w), x, 'conv3x3_phased')
    if relu_mask is not None and relu_mask.shape != out.shape:
        raise L.TecoganHipError('conv3x3_phased: relu_mask shape mismatch')
    ks = 1 if relu_mask is not None else L.lib().tg_conv3x3_phased_pick_ksplit(n, cin, cout, h, w, ocb)
    taps = (int(tapsel), int(cphase), int(taps_phase0), int(taps_phase1))
    if ks > 1:          # too few tiles for the device: channel chunks split over ks workgroup sets + finalize
        part = torch.empty(ks * n * cout * h * w, dtype=torch.float32, device=x.device)
        _call('tg_conv3x3_fwd_phased_splitk', x.data_ptr(), cin * h * w, wpk.data_ptr(), ocb, None, out.data_ptr(),
              n, cin, cout, h, w, ACT_NONE, *taps, ks, part.data_ptr())
        return out
    _call('tg_conv3x3_fwd_phased_masked', x.data_ptr(), cin * h * w, wpk.data_ptr(), ocb, None, _ptr(relu_mask),
          cout * h * w, out.data_ptr(), cout * h * w, n, cin, cout, h, w, ACT_NONE, *taps)
    return out


def pack_conv3x3_m16(weight, transposed=0):
    """tg_conv3x3_pack16: the A-operand layout of the 16 x 16 x 4 chained kernel (cin, cout <= 64);
    transposed = 2: the data gradient (channel roles swapped, taps rotated)."""
    w = _chk(weight, 'weight').detach()
    cout, cin = w.shape[0], w.shape[1]
    out = torch.empty(L.lib().tg_conv3x3_pack16_floats(), dtype=torch.float32, device=w.device)
    cin, cout, transposed = (cout, cin, 2) if transposed == 2 else (cin, cout, 0)
    _call('tg_conv3x3_pack16', w.data_ptr(), out.data_ptr(), cin, cout, transposed)
    return out


def chain_pack(items, layout):
    """tg_conv3x3_chain_pack: items = [(weight (O, I_total, 3, 3), i_off, i_cnt, transposed)] -> list of packed
    tensors (views of one buffer) in the chained kernels' layout `layout` (16 | 64), ONE launch."""
    lib = L.lib()
    arr = (L.PackItem * len(items))()
    sizes = []
    for wt, i_off, i_cnt, tr in items:
        _chk(wt, 'weight')
        cin, cout = (wt.shape[0], i_cnt) if tr == 2 else (i_cnt, wt.shape[0])
        sizes.append(int(lib.tg_conv3x3_chain_packed_floats(layout, cin)))
    buf = torch.empty(sum(sizes), dtype=torch.float32, device=items[0][0].device)
    outs, off = [], 0
    for a, (wt, i_off, i_cnt, tr), sz in zip(arr, items, sizes):
        o = buf[off:off + sz]; off += sz
        outs.append(o)
        a.w, a.out, a.transposed, a.i_total, a.i_off = wt.data_ptr(), o.data_ptr(), tr, wt.shape[1], i_off
        a.cin, a.cout = (wt.shape[0], i_cnt) if tr == 2 else (i_cnt, wt.shape[0])
    _call('tg_conv3x3_chain_pack', arr, len(items), layout)
    return outs


def conv3x3s2_supported(n, cin, cout, h_out, w_out):
    return bool(L.lib().tg_conv3x3s2_supported(n, cin, cout, h_out, w_out))


def conv3x3s2(x, wpk, cin, cout, relu_mask=None, out=None):
    """Stride-2 3x3 conv (tg_conv3x3s2_fwd): x (n, cin, 2h, 2w) -> (n, cout, h, w); the data gradient of
    ConvTranspose2d(k3, s2, p1, op1) with wpk = pack_conv3x3(W viewed as (cout = ci, cin = co), ocb 64)."""
    _chk_all(x=x, wpk=wpk)
    _chk_opt(relu_mask=relu_mask)
    n, c, h2, w2 = x.shape
    if c != cin or h2 % 2 or w2 % 2:
        raise L.TecoganHipError(f'conv3x3s2: x {tuple(x.shape)} cin {cin}')
    h, w = h2 // 2, w2 // 2
    out = _out(out, (n, cout, h, w), x, 'conv3x3s2')
    if relu_mask is not None and relu_mask.shape != out.shape:
        raise L.TecoganHipError('conv3x3s2: relu_mask shape mismatch')
    _call('tg_conv3x3s2_fwd', x.data_ptr(), cin * h2 * w2, wpk.data_ptr(), None, _ptr(relu_mask), cout * h * w,
          out.data_ptr(), cout * h * w, n, cin, cout, h, w, ACT_NONE)
    return out


def convt3x3s2(x, wpk, bias, cout, act=ACT_NONE, out=None):
    _chk_all(x=x, wpk=wpk)
    _chk_opt(bias=bias)
    n, cin, h, w = x.shape
    out = _out(out, (n, cout, 2 * h, 2 * w), x, 'convt3x3s2')
    _call('tg_convt3x3s2_fwd', x.data_ptr(), cin * h * w, wpk.data_ptr(), _ptr(bias), out.data_ptr(), cout * 4 * h * w,
          n, cin, cout, h, w, act)
    return out


def convt_pack_wz(w_out_oihw):
    """tg_convt_pack_wz: the output conv's (cz, nf, 3, 3) weight as the A operand of the Z-mode contraction."""
    _chk(w_out_oihw, 'w_out')
    cz, nf = w_out_oihw.shape[:2]
    wz = torch.empty(2 * 16 * 64, dtype=torch.float32, device=w_out_oihw.device)
    _call('tg_convt_pack_wz', w_out_oihw.data_ptr(), wz.data_ptr(), cz, nf)
    return wz


def convt3x3s2_z(x, wpk, bias, wz, cz, cout, act=ACT_NONE, form=-1, out=None):
    """tg_convt3x3s2_z_fwd_form: ConvTranspose2d(cin, cout, 3, 2, 1, 1) + act with the following 3x3 output conv's
    channel contraction in the epilogue -> (n, 32, 2h, 2w) buffer whose first 9 * cz planes are the output conv's tap
    planes (tecogan_nets.py:119-131).  form: -1 the library's rule, 0 tiled in one launch, 3 tiled with a split tail (all
    bit-identical); any other value raises TecoganHipError (1 and 2 were a streaming form that lost its A/B and was
    removed: EXPERIMENTS.md, round 6)."""
    _chk_all(x=x, wpk=wpk, wz=wz)
    _chk_opt(bias=bias)
    n, cin, h, w = x.shape
    out = _out(out, (n, 32, 2 * h, 2 * w), x, 'convt3x3s2_z')
    _call('tg_convt3x3s2_z_fwd_form', x.data_ptr(), cin * h * w, wpk.data_ptr(), _ptr(bias), wz.data_ptr(), cz,
          out.data_ptr(), 32 * 4 * h * w, n, cin, cout, h, w, act, form)
    return out


def convt_pack_wino(wpk, cin, cout):
    """tg_convt_pack_wino: the 16 Winograd-domain weight matrices of tg_convt3x3s2_z_wino_fwd from the direct form's
    packed ConvTranspose2d weights (pack_conv3x3(weight, transposed=True)[0])."""
    _chk(wpk, 'wpk')
    wa = torch.empty(L.TG_CONVT_WINO_FLOATS, dtype=torch.float32, device=wpk.device)
    _call('tg_convt_pack_wino', wpk.data_ptr(), wa.data_ptr(), cin, cout)
    return wa


def convt3x3s2_z_wino(x, wa, bias, wz, cz, cout, act=ACT_NONE, split=-1, out=None):
    """tg_convt3x3s2_z_wino_fwd: the tap planes of convt3x3s2_z computed in the Winograd domain (F(2,2) along x and y,
    25 products per 2x2 input tile instead of 36).  wa: convt_pack_wino.  split: -1 the library's rule, 0 one launch,
    1 whole rounds of workgroups + a remainder launch (bit-identical)."""
    _chk_all(x=x, wa=wa, wz=wz)
    _chk_opt(bias=bias)
    n, cin, h, w = x.shape
    out = _out(out, (n, 32, 2 * h, 2 * w), x, 'convt3x3s2_z_wino')
    _call('tg_convt3x3s2_z_wino_fwd', x.data_ptr(), cin * h * w, wa.data_ptr(), _ptr(bias), wz.data_ptr(), cz,
          out.data_ptr(), 32 * 4 * h * w, n, cin, cout, h, w, act, split)
    return out


def convout_tail(z, cz, bias, up_src=None, up_mode=UP_NONE, up_scale=1, want_u8=False, form=-1):
    """tg_convout_tail_form: out[o] = bias[o] + sum_tap z[tap * cz + o] shifted by the tap (zero padding) [+ the
    up-sampled residual of up_src] -> fp32 (n, cz, h, w) [and the uint8 (n, h, w, cz) frame].  z: (n, 32, h, w) planes
    of tg_convt3x3s2_z_fwd.  form: -1 the library's rule, 0 one pixel per thread, 1 four (bit-identical)."""
    _chk(z, 'z')
    _chk_opt(bias=bias, up_src=up_src)
    n, _, h, w = z.shape
    y = torch.empty(n, cz, h, w, dtype=torch.float32, device=z.device)
    u8 = torch.empty(n, h, w, cz, dtype=torch.uint8, device=z.device) if want_u8 else None
    _call('tg_convout_tail_form', z.data_ptr(), z.shape[1] * h * w, cz, _ptr(bias), _ptr(up_src), up_mode, up_scale,
          y.data_ptr(), cz * h * w, _ptr(u8), n, h, w, form)
    return (y, u8) if want_u8 else y


def conv3x3_fewin_ok(x, cout, any_size=False):
    """whether tg_conv3x3_fewin_fwd takes the launch -- and pays: below one 4 x 64 tile per CU the MFMA
    kernel is faster (2 x 128 x 128: 8.7 against 11.2 us; 2 x 256 x 256: 27.9 against 18.8 us)"""
    n, cin, h, w = x.shape
    ok = cin <= 4 and w % 4 == 0 and x.data_ptr() % 16 == 0 and (cin * h * w) % 4 == 0 and (cout * h * w) % 4 == 0
    return ok and (any_size or n * ((h + 3) // 4) * ((w + 63) // 64) >= 256)


def conv3x3_fewin(x, w_oihw, relu_mask=None, out=None):
    """tg_conv3x3_fewin_fwd: 3x3 conv from <= 4 input channels (w_oihw: (cout, cin, 3, 3)), no bias /
    activation, y = relu_mask > 0 ? conv : 0 -- the data gradient of a small-cout head."""
    _chk_all(x=x, weight=w_oihw)
    _chk_opt(relu_mask=relu_mask)
    n, cin, h, w = x.shape
    cout = w_oihw.shape[0]
    if tuple(w_oihw.shape) != (cout, cin, 3, 3):
        raise L.TecoganHipError(f'conv3x3_fewin: weight {tuple(w_oihw.shape)} for {cin} input channels')
    out = _out(out, (n, cout, h, w), x, 'conv3x3_fewin')
    if relu_mask is not None and relu_mask.shape != out.shape:
        raise L.TecoganHipError('conv3x3_fewin: relu_mask shape mismatch')
    _call('tg_conv3x3_fewin_fwd', x.data_ptr(), cin * h * w, w_oihw.data_ptr(), _ptr(relu_mask), cout * h * w,
          out.data_ptr(), cout * h * w, n, cin, cout, h, w)
    return out


def conv3x3_small_res_ok(x, res):
    """whether tg_conv3x3_small_fwd_res takes this launch (w % 4 == 0, aligned planes)"""
    return x.shape[3] % 4 == 0 and x.data_ptr() % 16 == 0 and res.data_ptr() % 16 == 0 and \
        (x.shape[1] * x.shape[2] * x.shape[3]) % 4 == 0 and (res.shape[1] * res.shape[2] * res.shape[3]) % 4 == 0


def conv3x3_small(x, weight, bias, act=ACT_NONE, up_src=None, up_mode=UP_NONE, up_scale=1,
                  out=None, res=None):
    _chk(x, 'x')
    w_ = _chk(weight, 'weight').detach()
    _chk_opt(bias=bias, up_src=up_src, res=res)
    n, cin, h, w = x.shape
    cout = w_.shape[0]
    out = _out(out, (n, cout, h, w), x, 'conv3x3_small')
    if res is not None:         # explicit residual tensor instead of an up-sampled source
        if up_src is not None or tuple(res.shape) != (n, cout, h, w):
            raise L.TecoganHipError('conv3x3_small: res must be (n, cout, h, w) and excludes up_src')
        _call('tg_conv3x3_small_fwd_res', x.data_ptr(), cin * h * w, w_.data_ptr(), _ptr(bias), res.data_ptr(),
              cout * h * w, out.data_ptr(), cout * h * w, n, cin, cout, h, w, act)
        return out
    _call('tg_conv3x3_small_fwd', x.data_ptr(), cin * h * w, w_.data_ptr(), _ptr(bias), _ptr(up_src), up_mode, up_scale,
          out.data_ptr(), cout * h * w, n, cin, cout, h, w, act)
    return out


def flowup_warp_s2d(lr_flow, hr_prev, h, w, scale, up_mode, out=None, want_hr_flow=False):
    _chk_all(lr_flow=lr_flow, hr_prev=hr_prev)
    n, c = hr_prev.shape[:2]
    fh, fw = lr_flow.shape[2:]
    out = _out(out, (n, scale * scale * c, h, w), hr_prev, 'flowup_warp_s2d')
    hr_flow = (torch.empty(n, 2, scale * h, scale * w, dtype=torch.float32, device=hr_prev.device)
               if want_hr_flow else None)
    _call('tg_flowup_warp_s2d_fwd', lr_flow.data_ptr(), fh, fw, hr_prev.data_ptr(), out.data_ptr(),
          scale * scale * c * h * w, _ptr(hr_flow), n, c, h, w, scale, up_mode)
    return (out, hr_flow) if want_hr_flow else out


def backward_warp(x, flow):
    _chk_all(x=x, flow=flow)
    n, c, h, w = x.shape
    if flow.shape != (n, 2, h, w):
        raise L.TecoganHipError(f'backward_warp: flow {tuple(flow.shape)} vs x {tuple(x.shape)}')
    out = torch.empty_like(x)
    _call('tg_backward_warp_fwd', x.data_ptr(), flow.data_ptr(), out.data_ptr(), n, c, h, w)
    return out


def backward_warp_s2d(x, flow, scale):
    """space_to_depth(backward_warp(x, flow), scale) in one launch (tg_backward_warp_s2d_fwd)."""
    _chk_all(x=x, flow=flow)
    n, c, h, w = x.shape
    if flow.shape != (n, 2, h, w) or h % scale or w % scale:
        raise L.TecoganHipError(f'backward_warp_s2d: flow {tuple(flow.shape)} vs x {tuple(x.shape)}, scale {scale}')
    out = torch.empty(n, scale * scale * c, h // scale, w // scale, dtype=torch.float32, device=x.device)
    _call('tg_backward_warp_s2d_fwd', x.data_ptr(), flow.data_ptr(), out.data_ptr(), n, c, h, w, scale)
    return out


def space_to_depth(x, scale):
    _chk(x, 'x')
    n, c, h, w = x.shape
    oh, ow = h // scale, w // scale
    out = torch.empty(n, scale * scale * c, oh, ow, dtype=torch.float32, device=x.device)
    _call('tg_space_to_depth', x.data_ptr(), out.data_ptr(), scale * scale * c * oh * ow, n, c, h, w, scale)
    return out


def upsample(x, scale, up_mode, mul=1.0):
    _chk(x, 'x')
    n, c, h, w = x.shape
    out = torch.empty(n, c, h * scale, w * scale, dtype=torch.float32, device=x.device)
    _call('tg_upsample_fwd', x.data_ptr(), out.data_ptr(), n * c, h, w, scale, up_mode, float(mul))
    return out


def maxpool2(x):
    _chk(x, 'x')
    n, c, h, w = x.shape
    out = torch.empty(n, c, h // 2, w // 2, dtype=torch.float32, device=x.device)
    _call('tg_maxpool2_fwd', x.data_ptr(), out.data_ptr(), n * c, h, w)
    return out


def quantize_u8_hwc(x):
    """(c,h,w) fp32 -> (h,w,c) uint8 on device."""
    _chk(x, 'x')
    c, h, w = x.shape
    out = torch.empty(h, w, c, dtype=torch.uint8, device=x.device)
    _call('tg_quantize_u8_hwc', x.data_ptr(), out.data_ptr(), c, h, w)
    return out


def dequantize_u8_hwc(x):
    """(n,h,w,c) uint8 on device -> (n,c,h,w) fp32 in [0,1] (= permute + float + /255)."""
    _chk_u8(x, 'x')
    n, h, w, c = x.shape
    out = torch.empty(n, c, h, w, dtype=torch.float32, device=x.device)
    _call('tg_dequantize_u8_hwc', x.data_ptr(), out.data_ptr(), n, c, h, w)
    return out


# -- planar YUV 4:2:0 | 4:2:2 | 4:4:4 at 8 | 10 | 12 bits, BT.601 | BT.709 | BT.2020 (DESIGN.md sections 7e, 7k, 7l): seven
# wrappers over seven entry points, one body per direction --------------------------------------------------------------
YUV_SUBSAMPLING = {'420': (2, 2), '422': (2, 1), '444': (1, 1)}     # chroma -> (sx, sy): luma samples per chroma sample


def yuv_frame_samples(h, w, chroma='420'):
    """Samples of one planar frame: Y h*w, then U and V of ceil(h/sy) x ceil(w/sx); chroma '420' | '422' | '444'."""
    if chroma not in YUV_SUBSAMPLING:
        raise L.TecoganHipError(f'yuv_frame_samples: chroma is one of {sorted(YUV_SUBSAMPLING)}, got {chroma!r}')
    sx, sy = YUV_SUBSAMPLING[chroma]
    return h * w + 2 * ((h + sy - 1) // sy) * ((w + sx - 1) // sx)


def yuv420_frame_bytes(h, w):
    """Bytes of one I420 frame, and 16-bit samples of one 10- or 12-bit I420 frame (2 bytes each)."""
    return yuv_frame_samples(h, w, '420')


yuv420p_frame_samples = yuv420_frame_bytes


def _yuv_codes(what, matrices, matrix, full_range, siting, chroma=None):
    """Names -> the C enums, (matrix, full_range, siting) with the chroma code in front if one is given; integers pass
    through (the library refuses an unknown value with TG_E_ARG)."""
    codes = []
    for name, val, table in (('chroma', chroma, L.YUV_CHROMA), ('matrix', matrix, matrices), ('siting', siting, L.YUV_SITING)):
        if isinstance(val, str) and val not in table:
            raise L.TecoganHipError(f'{what}: {name} is one of {sorted(table)}, got {val!r}')
        if val is not None:
            codes.append(table[val] if isinstance(val, str) else int(val))
    return (*codes[:-1], int(full_range), codes[-1])


def _chk_depth(depth, what, depths='10 or 12'):
    if isinstance(depth, bool) or not isinstance(depth, int):
        raise L.TecoganHipError(f'{what}: depth is {depths}, got {depth!r}')
    return depth


def _yuv_in(what, launch, yuv, dtype, h, w, ns, frames, lead, out=None):
    """The input direction's one body: (n, ns) / (ns,) samples of `dtype` on device -> (n,3,h,w) fp32 through
    `launch`(yuv, out, n, h, w, *lead, stream).  ns None: a layout the wrapper does not know, which the library refuses
    before any access."""
    _chk(yuv, 'yuv', dtype)
    if yuv.dim() == 1:
        yuv = yuv.unsqueeze(0)
    if ns is not None and (yuv.dim() != 2 or yuv.shape[1] != ns):
        raise L.TecoganHipError(f'{what}: {h}x{w} {frames}; got shape {tuple(yuv.shape)}')
    n = yuv.shape[0]
    out = _out(out, (n, 3, h, w), yuv, what)
    _call(launch, _ptr(yuv), _ptr(out), n, h, w, *lead)
    return out


def _yuv_out(what, launch, rgb, deep, chroma, lead, out=None):
    """The output direction's one body: (n,H,W,3) uint8 RGB -> (n, frame_samples) uint8, or with `deep` (n,3,H,W) float32
    RGB -> uint16, through `launch`(rgb, out, n, H, W, *lead, stream)."""
    _chk(rgb, 'rgb', torch.float32 if deep else torch.uint8)
    if rgb.dim() != 4 or rgb.shape[1 if deep else 3] != 3:
        raise L.TecoganHipError(f'{what}: expected {"(n,3,H,W)" if deep else "(n,H,W,3)"}, got shape {tuple(rgb.shape)}')
    n, H, W = (rgb.shape[0], *rgb.shape[2:]) if deep else rgb.shape[:3]
    out = _out(out, (n, yuv_frame_samples(H, W, chroma)), rgb, what, torch.uint16 if deep else torch.uint8)
    _call(launch, _ptr(rgb), _ptr(out), n, H, W, *lead)
    return out


def yuv420_to_rgb(yuv, h, w, matrix='bt709', full_range=False, siting='left'):
    """(n, frame_bytes) / (frame_bytes,) uint8 I420 frames on device -> (n,3,h,w) fp32 RGB in [0,1]: integer bilinear
    chroma up-sampling, one fp32 matrix step, clamp (tg_yuv420_to_rgb_f32)."""
    ns = yuv420_frame_bytes(h, w)
    return _yuv_in('yuv420_to_rgb', 'tg_yuv420_to_rgb_f32', yuv, torch.uint8, h, w, ns, f'frames have {ns} bytes',
                   _yuv_codes('yuv420_to_rgb', L.YUV_MATRIX, matrix, full_range, siting))


def rgb_to_yuv420(rgb_hwc, matrix='bt709', full_range=False, siting='left'):
    """(n,H,W,3) uint8 RGB on device -> (n, frame_bytes) uint8 I420 frames, exact integer arithmetic; H and W even
    (tg_rgb_u8_to_yuv420)."""
    return _yuv_out('rgb_to_yuv420', 'tg_rgb_u8_to_yuv420', rgb_hwc, False, '420',
                    _yuv_codes('rgb_to_yuv420', L.YUV_MATRIX, matrix, full_range, siting))


def yuv420p_to_rgb(yuv_u16, h, w, depth, matrix='bt709', full_range=False, siting='left', out=None):
    """(n, frame_samples) / (frame_samples,) uint16 I420 frames at `depth` (10 | 12) bits on device -> (n,3,h,w) fp32
    RGB in [0,1]; a sample above 2^depth - 1 is read as 2^depth - 1 (tg_yuv420p16_to_rgb_f32).
    out: a contiguous CUDA float32 (n,3,h,w) tensor to write into."""
    ns = yuv420p_frame_samples(h, w)
    return _yuv_in('yuv420p_to_rgb', 'tg_yuv420p16_to_rgb_f32', yuv_u16, torch.uint16, h, w, ns, f'frames have {ns} samples',
                   (_chk_depth(depth, 'yuv420p_to_rgb'), *_yuv_codes('yuv420p_to_rgb', L.YUV_MATRIX, matrix, full_range, siting)),
                   out)


def rgb_f32_to_yuv420p(rgb_chw, depth, matrix='bt709', full_range=False, siting='left', out=None):
    """(n,3,H,W) float32 RGB on device -> (n, frame_samples) uint16 I420 frames at `depth` (10 | 12) bits: one fp32
    step to 16-bit integers, then exact integer arithmetic; H and W even (tg_rgb_f32_to_yuv420p16; DESIGN.md section
    7k).  out: a contiguous CUDA uint16 (n, frame_samples) tensor to write into."""
    return _yuv_out('rgb_f32_to_yuv420p', 'tg_rgb_f32_to_yuv420p16', rgb_chw, True, '420',
                    (_chk_depth(depth, 'rgb_f32_to_yuv420p'),
                     *_yuv_codes('rgb_f32_to_yuv420p', L.YUV_MATRIX, matrix, full_range, siting)), out)


def yuv_to_rgb(yuv, h, w, chroma='420', depth=8, matrix='bt709', full_range=False, siting='left', out=None):
    """(n, frame_samples) / (frame_samples,) planar YUV frames on device -- uint8 at depth 8, uint16 at 10 | 12 --
    -> (n,3,h,w) fp32 RGB in [0,1] (tg_yuv_planar_to_rgb_f32).  chroma '420' | '422' | '444',
    matrix 'bt601' | 'bt709' | 'bt2020'.  out: a contiguous CUDA float32 (n,3,h,w) tensor to write into."""
    _chk_depth(depth, 'yuv_to_rgb', '8, 10 or 12')
    c, m, r, s = _yuv_codes('yuv_to_rgb', L.YUV_PLANAR_MATRIX, matrix, full_range, siting, chroma)
    chroma = {v: k for k, v in L.YUV_CHROMA.items()}.get(c)          # (None: the library refuses it before any access)
    ns = None if chroma is None else yuv_frame_samples(h, w, chroma)
    return _yuv_in('yuv_to_rgb', 'tg_yuv_planar_to_rgb_f32', yuv, torch.uint8 if depth == 8 else torch.uint16, h, w, ns,
                   f'{chroma} frames have {ns} samples', (c, depth, m, r, s), out)


def rgb_to_yuv(rgb_hwc, chroma='420', matrix='bt709', full_range=False, siting='left'):
    """(n,H,W,3) uint8 RGB on device -> (n, frame_samples) uint8 planar YUV frames, exact integer arithmetic
    (tg_rgb_u8_to_yuv_planar).  '420': H and W even; '422': W even; '444': any size."""
    if not isinstance(chroma, str):
        raise L.TecoganHipError(f'rgb_to_yuv: chroma is one of {sorted(L.YUV_CHROMA)}, got {chroma!r}')
    return _yuv_out('rgb_to_yuv', 'tg_rgb_u8_to_yuv_planar', rgb_hwc, False, chroma,
                    _yuv_codes('rgb_to_yuv', L.YUV_PLANAR_MATRIX, matrix, full_range, siting, chroma))


def rgb_f32_to_yuv(rgb_chw, chroma='420', depth=10, matrix='bt709', full_range=False, siting='left', out=None):
    """(n,3,H,W) float32 RGB on device -> (n, frame_samples) uint16 planar YUV frames at `depth` (10 | 12) bits: one
    fp32 step to 16-bit integers, then exact integer arithmetic (tg_rgb_f32_to_yuv_planar16).
    The sizes of rgb_to_yuv.  out: a contiguous CUDA uint16 (n, frame_samples) tensor to write into."""
    if not isinstance(chroma, str):
        raise L.TecoganHipError(f'rgb_f32_to_yuv: chroma is one of {sorted(L.YUV_CHROMA)}, got {chroma!r}')
    c, m, r, s = _yuv_codes('rgb_f32_to_yuv', L.YUV_PLANAR_MATRIX, matrix, full_range, siting, chroma)
    return _yuv_out('rgb_f32_to_yuv', 'tg_rgb_f32_to_yuv_planar16', rgb_chw, True, chroma,
                    (c, _chk_depth(depth, 'rgb_f32_to_yuv'), m, r, s), out)


DEINTERLACE_RATES = {'field': 1, 'frame': 2}       # rate -> the field step of tg_deinterlace_planar


def deinterlace(frames, h, w, chroma='420', depth=8, tff=True, rate='field', prev=None, out=None):
    """(k, frame_samples) interlaced planar YUV frames on device -- uint8 at depth 8, uint16 at 10 | 12 -- -> progressive
    frames of the same layout: (2k, frame_samples) at rate 'field' (both fields of every frame, in time order), (k,
    frame_samples) at rate 'frame' (the earlier field's frame only).  Edge-directed line average bounded by a three-field
    motion measure, exact integers (tg_deinterlace_planar; the specification is
    tests/deinterlace_ref.py).  tff: the earlier field owns the even rows.  prev: the frame before frames[0], (frame_samples,)
    or (1, frame_samples), or None: the two outputs of frames[0] are then spatial only.  h is even (a multiple of 4 at
    '420').  out: a contiguous CUDA tensor of the result's shape and type to write into."""
    _chk_depth(depth, 'deinterlace', '8, 10 or 12')
    if not isinstance(chroma, str) or chroma not in L.YUV_CHROMA:
        raise L.TecoganHipError(f'deinterlace: chroma is one of {sorted(L.YUV_CHROMA)}, got {chroma!r}')
    if rate not in DEINTERLACE_RATES:
        raise L.TecoganHipError(f'deinterlace: rate is one of {sorted(DEINTERLACE_RATES)}, got {rate!r}')
    dtype = torch.uint8 if depth == 8 else torch.uint16
    ns = yuv_frame_samples(h, w, chroma)
    _chk(frames, 'frames', dtype)
    _chk_opt(dtype, prev=prev)
    if frames.dim() != 2 or frames.shape[0] < 1 or frames.shape[1] != ns:
        raise L.TecoganHipError(f'deinterlace: {h}x{w} {chroma} frames are (k, {ns}); got shape {tuple(frames.shape)}')
    k, step = frames.shape[0], DEINTERLACE_RATES[rate]
    cnt = 2 * k // step
    if prev is not None and prev.numel() != ns:
        raise L.TecoganHipError(f'deinterlace: prev is one frame of {ns} samples; got shape {tuple(prev.shape)}')
    out = _out(out, (cnt, ns), frames, 'deinterlace', dtype)
    # the entry point takes the frame before and the k frames as one run of memory
    run = torch.empty(k + 1, ns, dtype=dtype, device=frames.device)
    run[1:].view(torch.uint8).copy_(frames.view(torch.uint8))
    if prev is not None:
        run[0].view(torch.uint8).copy_(prev.reshape(ns).view(torch.uint8))
    _call('tg_deinterlace_planar', _ptr(run), _ptr(out), k, h, w, L.YUV_CHROMA[chroma], depth, 1 if tff else 0,
          0 if prev is None else 1, 0, step, cnt)
    return out


def png_encode(rgb_hwc, filter='adaptive', lz77=False):
    """(n,H,W,3) / (H,W,3) uint8 RGB on device -> a list of n host `bytes`, each one complete PNG file, encoded on
    the device (tg_png_encode_u8): filter 'adaptive' | 'none', Huffman-only deflate in segments
    of 32768 bytes, the bytes of tests/png_ref.py.  lz77=True: tg_png_encode_lz_u8 (section 7n), LZ77 matches inside a
    segment, the bytes of tests/png_lz_ref.py, never more than without it.  Synchronises: for tools and tests; a
    stream writes files through FRNet.infer_stream(png=...)."""
    if not isinstance(lz77, bool):
        raise L.TecoganHipError(f'png_encode: lz77 is True or False, got {lz77!r}')
    _chk_u8(rgb_hwc, 'rgb')
    if rgb_hwc.dim() == 3:
        rgb_hwc = rgb_hwc.unsqueeze(0)
    if rgb_hwc.dim() != 4 or rgb_hwc.shape[3] != 3 or rgb_hwc.shape[0] < 1:
        raise L.TecoganHipError(f'png_encode: expected (n,H,W,3) or (H,W,3), got shape {tuple(rgb_hwc.shape)}')
    if isinstance(filter, str) and filter not in L.PNG_FILTER:
        raise L.TecoganHipError(f'png_encode: filter is one of {sorted(L.PNG_FILTER)}, got {filter!r}')
    code = L.PNG_FILTER[filter] if isinstance(filter, str) else int(filter)
    n, H, W, _ = rgb_hwc.shape
    lib, dev = L.lib(), rgb_hwc.device
    name, ws_name = ('tg_png_encode_lz_u8', 'tg_png_lz_workspace_bytes') if lz77 else \
        ('tg_png_encode_u8', 'tg_png_workspace_bytes')
    cap, wsb = lib.tg_png_capacity(H, W), getattr(lib, ws_name)(n, H, W)
    if cap < 0 or wsb < 0:
        L.check(L.TG_E_SHAPE, 'tg_png_capacity')
    out = torch.empty(n, cap, dtype=torch.uint8, device=dev)
    sizes = torch.empty(n, dtype=torch.int64, device=dev)
    ws = _workspace(wsb, dev)
    _call(name, _ptr(rgb_hwc), n, H, W, code, _ptr(out), cap, _ptr(sizes), _ptr(ws))
    sizes, out = sizes.cpu().tolist(), out.cpu().numpy()
    return [out[k, :sizes[k]].tobytes() for k in range(n)]


def scene_cut_flags(frames, mad, hist, forced=None, detect=True):
    """(n+1,3,h,w) fp32 frames on device -> (flags int32 (n,), sad int64 (n,), hdist int32 (n,)): pair j is frame
    j + 1 against frame j.  sad = sum |dY| of the 8-bit lumas, hdist = L1 distance of their 32-bin histograms, flag =
    forced[j] or (detect and sad >= ceil(mad h w) and hdist >= ceil(hist 2 h w)), exact integers (tg_scene_cut_flags;
    DESIGN.md section 7h).  forced: n values, non-zero = cut whatever the detector says.  For tests and for tuning the
    thresholds: sad / (h w) and hdist / (2 h w) are the scores SceneCut(keep_scores=True) reports."""
    _chk(frames, 'frames')
    if frames.dim() != 4 or frames.shape[0] < 2 or frames.shape[1] != 3:
        raise L.TecoganHipError(f'scene_cut_flags: expected (n+1,3,h,w) with n >= 1, got shape {tuple(frames.shape)}')
    if not (math.isfinite(mad) and math.isfinite(hist) and mad >= 0 and hist >= 0):
        raise L.TecoganHipError(f'scene_cut_flags: mad and hist are finite and >= 0, got {mad!r}, {hist!r}')
    n, (h, w), dev = frames.shape[0] - 1, frames.shape[2:], frames.device
    top = 2 ** 64 - 1
    s_min, d_min = min(top, math.ceil(mad * h * w)), min(top, math.ceil(hist * 2 * h * w))
    if forced is not None:      # any sequence of values: the uint8 table is built here
        forced = torch.as_tensor(forced).reshape(-1).ne(0).to(torch.uint8).to(dev).contiguous()
        if forced.numel() != n:
            raise L.TecoganHipError(f'scene_cut_flags: forced has {forced.numel()} entries for {n} pairs')
    flags = torch.empty(n, dtype=torch.int32, device=dev)
    sad = torch.empty(n, dtype=torch.int64, device=dev)
    hdist = torch.empty(n, dtype=torch.int32, device=dev)
    ws = _workspace(L.lib().tg_scene_cut_workspace_bytes(n), dev)
    _call('tg_scene_cut_flags', _ptr(frames), n, h, w, s_min, d_min, _ptr(forced), 1 if detect else 0, _ptr(flags),
          _ptr(sad), _ptr(hdist), _ptr(ws), ws.numel())
    return flags, sad, hdist


def psnr_sse_u8(true_hwc, pred_hwc, y_only=True):
    """Per-frame sum of squared differences of (t,h,w,3) uint8 device tensors -> int64 (t,)."""
    _chk_u8(true_hwc, 'true'); _chk_u8(pred_hwc, 'pred')
    if true_hwc.shape != pred_hwc.shape or true_hwc.dim() != 4 or true_hwc.shape[3] != 3:
        raise L.TecoganHipError(f'psnr_sse_u8: shapes {tuple(true_hwc.shape)} / {tuple(pred_hwc.shape)}')
    t, h, w, _ = true_hwc.shape
    sse = torch.empty(t, dtype=torch.int64, device=true_hwc.device)
    _call('tg_psnr_sse_u8', true_hwc.data_ptr(), pred_hwc.data_ptr(), sse.data_ptr(), t, h, w, 1 if y_only else 0)
    return sse


def luma_u8(rgb):
    """(n,3) uint8 -> (n,) uint8, the Y channel of rgb_to_ycbcr."""
    _chk_u8(rgb, 'rgb')
    out = torch.empty(rgb.shape[0], dtype=torch.uint8, device=rgb.device)
    _call('tg_luma_u8', rgb.data_ptr(), out.data_ptr(), rgb.shape[0])
    return out


def lpips_conv(x0, wt, bias, cout, ks, stride, pad, x1=None, lut=None, out=None):
    """tg_lpips_conv_fwd: relu(Conv2d(cin, cout, ks, stride, pad)(cat[x0, x1]) + bias).
    lut given: x0 / x1 are (n,h,w,3) uint8 images read through the (256,3) table; else (n,cin,h,w) fp32.
    wt: (cin*ks*ks, cout), the Conv2d weight reshaped to (cout, K) and transposed."""
    _chk_all(wt=wt, bias=bias)
    if lut is not None:
        _chk(lut, 'lut'); _chk_u8(x0, 'x0')
        if x1 is not None:
            _chk_u8(x1, 'x1')
        n0, h, w, cin = x0.shape
    else:
        _chk(x0, 'x0')
        _chk_opt(x1=x1)
        n0, cin, h, w = x0.shape
    if x1 is not None and tuple(x1.shape[1:]) != tuple(x0.shape[1:]):
        raise L.TecoganHipError(f'lpips_conv: x0 {tuple(x0.shape)} x1 {tuple(x1.shape)}')
    if tuple(wt.shape) != (cin * ks * ks, cout) or tuple(bias.shape) != (cout,):
        raise L.TecoganHipError(f'lpips_conv: wt {tuple(wt.shape)} bias {tuple(bias.shape)} for cin {cin} '
                                f'cout {cout} k{ks}')
    n = n0 + (0 if x1 is None else x1.shape[0])
    oh, ow = (h + 2 * pad - ks) // stride + 1, (w + 2 * pad - ks) // stride + 1
    out = _out(out, (n, cout, oh, ow), x0, 'lpips_conv')
    _call('tg_lpips_conv_fwd', x0.data_ptr(), _ptr(x1), n0, _ptr(lut), wt.data_ptr(), bias.data_ptr(), out.data_ptr(),
          n, cin, h, w, cout, ks, stride, pad)
    return out


def maxpool3s2(x, out=None):
    """nn.MaxPool2d(3, 2) (floor mode) of (n,c,h,w) fp32."""
    _chk(x, 'x')
    n, c, h, w = x.shape
    out = _out(out, (n, c, (h - 3) // 2 + 1, (w - 3) // 2 + 1), x, 'maxpool3s2')
    _call('tg_maxpool3s2_fwd', x.data_ptr(), out.data_ptr(), n * c, h, w)
    return out


def lpips_head(feat_true, feat_pred, lin, res, layer, total=None):
    """tg_lpips_head: one LPIPS layer of (t,c,h,w) feature maps into column `layer` of res (t,5);
    with total (t,) (layer 4 only): the sum of the five columns in order."""
    _chk_all(feat_true=feat_true, feat_pred=feat_pred, lin=lin, res=res)
    _chk_opt(total=total)
    t, c, h, w = feat_true.shape
    if feat_pred.shape != feat_true.shape or lin.numel() != c or tuple(res.shape) != (t, 5):
        raise L.TecoganHipError(f'lpips_head: feats {tuple(feat_true.shape)} / {tuple(feat_pred.shape)}, '
                                f'lin {tuple(lin.shape)}, res {tuple(res.shape)}')
    if total is not None and tuple(total.shape) != (t,):
        raise L.TecoganHipError(f'lpips_head: total {tuple(total.shape)}')
    ws = _workspace(L.lib().tg_lpips_head_workspace_bytes(t, h, w), feat_true.device)
    _call('tg_lpips_head', feat_true.data_ptr(), feat_pred.data_ptr(), lin.data_ptr(), t, c, h, w, ws.data_ptr(),
          res.data_ptr(), layer, _ptr(total))
    return res


def _window_args(true_hwc, pred_hwc, window, what):
    """Checks of the windowed frame metrics: (t,h,w,3) uint8 device frames, a window inside both."""
    _chk_u8(true_hwc, 'true'); _chk_u8(pred_hwc, 'pred')
    if true_hwc.dim() != 4 or pred_hwc.dim() != 4 or true_hwc.shape[3] != 3 or pred_hwc.shape[3] != 3 or \
            true_hwc.shape[0] != pred_hwc.shape[0] or true_hwc.shape[0] < 1:
        raise L.TecoganHipError(f'{what}: shapes {tuple(true_hwc.shape)} / {tuple(pred_hwc.shape)}')
    t, th, tw, _ = true_hwc.shape
    _, ph, pw, _ = pred_hwc.shape
    if window is None:
        if (th, tw) != (ph, pw):
            raise L.TecoganHipError(f'{what}: frames of {th}x{tw} and {ph}x{pw} need a window')
        window = (0, 0, th, tw)
    y0, x0, h, w = (int(v) for v in window)
    return t, th, tw, ph, pw, y0, x0, h, w


def ssim_y_u8(true_hwc, pred_hwc, window=None):
    """tg_ssim_y_u8: per-frame mean SSIM of the unrounded Y planes (7x7 uniform window, data_range of the
    predicted frame) of (t,h,w,3) uint8 device frames on window = (y0, x0, h, w), the same origin in both
    (None: the whole, equally sized frames) -> float64 (t,) on the device."""
    t, th, tw, ph, pw, y0, x0, h, w = _window_args(true_hwc, pred_hwc, window, 'ssim_y_u8')
    nbytes = L.lib().tg_ssim_workspace_bytes(t, h, w)
    if nbytes < 0:
        raise L.TecoganHipError(f'ssim_y_u8: no workspace for frames={t} window {h}x{w} (at least 7x7)')
    ws = _workspace(nbytes, true_hwc.device)
    out = torch.empty(t, dtype=torch.float64, device=true_hwc.device)
    _call('tg_ssim_y_u8', true_hwc.data_ptr(), pred_hwc.data_ptr(), t, th, tw, ph, pw, y0, x0, h, w, out.data_ptr(),
          ws.data_ptr(), ws.numel())
    return out


def psnr_yfloat_sse_u8(true_hwc, pred_hwc, window=None):
    """tg_psnr_yfloat_sse_u8: exact per-frame sums of (y'_true - y'_pred)^2 over the window, with the integer
    luma y' = 65481 R + 128553 G + 24966 B (Y = 16 + y' / 255000) -> list of t Python integers (a frame's sum
    does not fit 64 bits; the kernel's per-block partials are added here)."""
    t, th, tw, ph, pw, y0, x0, h, w = _window_args(true_hwc, pred_hwc, window, 'psnr_yfloat_sse_u8')
    nb = L.lib().tg_psnr_yfloat_partials(h, w)
    if nb < 0:
        raise L.TecoganHipError(f'psnr_yfloat_sse_u8: window {h}x{w}')
    part = torch.empty(t, nb, dtype=torch.int64, device=true_hwc.device)
    _call('tg_psnr_yfloat_sse_u8', true_hwc.data_ptr(), pred_hwc.data_ptr(), t, th, tw, ph, pw, y0, x0, h, w,
          part.data_ptr())
    # the partials are unsigned 64-bit (up to 4096 * 3.12e15 > 2^63): undo int64's wrap
    return [sum(v + (1 << 64) if v < 0 else v for v in row) for row in part.tolist()]


def farneback_levels(h, w):
    """[(lh, lw)] of pyramid levels 0..L of an h x w frame (tg_fb_level_size; no device work)."""
    lh, lw = ctypes.c_int(), ctypes.c_int()
    top = L.lib().tg_fb_level_size(h, w, 0, ctypes.byref(lh), ctypes.byref(lw))
    if top < 0:
        L.check(top, 'tg_fb_level_size')
    out = []
    for k in range(top + 1):
        L.lib().tg_fb_level_size(h, w, k, ctypes.byref(lh), ctypes.byref(lw))
        out.append((lh.value, lw.value))
    return out


def farneback_flow(frames_u8, size=None):
    """tg_farneback_flow_u8: (t, fh, fw, 3) uint8 device frames -> (t-1, h, w, 2) fp32 flows of the consecutive pairs
    (channel 0 = x), computed on the top-left size = (h, w) of the frames (None: the whole frames).  Farneback's
    method with the reference's fixed parameters as DESIGN.md section 7f restates it; not compared with OpenCV."""
    _chk_u8(frames_u8, 'frames')
    if frames_u8.dim() != 4 or frames_u8.shape[3] != 3 or frames_u8.shape[0] < 2:
        raise L.TecoganHipError(f'farneback_flow: frames {tuple(frames_u8.shape)} (at least two (h,w,3) frames)')
    t, fh, fw, _ = frames_u8.shape
    h, w = (fh, fw) if size is None else (int(size[0]), int(size[1]))
    nbytes = L.lib().tg_farneback_workspace_bytes(t - 1, h, w)
    if nbytes < 0 or h > fh or w > fw:
        raise L.TecoganHipError(f'farneback_flow: region {h}x{w} of {t} frames of {fh}x{fw} (at least 16x16, inside)')
    ws = _workspace(nbytes, frames_u8.device)
    out = torch.empty(t - 1, h, w, 2, dtype=torch.float32, device=frames_u8.device)
    _call('tg_farneback_flow_u8', frames_u8.data_ptr(), t, fh, fw, h, w, out.data_ptr(), ws.data_ptr(), ws.numel())
    return out


def flow_epe_mean(flow_a, flow_b, window=None):
    """tg_flow_epe_mean: (n, h, w, 2) fp32 flows -> float64 (n,) mean end-point errors over window = (y0, x0, h, w)
    (None: the whole field)."""
    _chk_all(flow_a=flow_a, flow_b=flow_b)
    if flow_a.dim() != 4 or flow_a.shape[3] != 2 or flow_a.shape != flow_b.shape or flow_a.shape[0] < 1:
        raise L.TecoganHipError(f'flow_epe_mean: flows {tuple(flow_a.shape)} / {tuple(flow_b.shape)}')
    n, h, w, _ = flow_a.shape
    y0, x0, ch, cw = (0, 0, h, w) if window is None else (int(v) for v in window)
    out = torch.empty(n, dtype=torch.float64, device=flow_a.device)
    _call('tg_flow_epe_mean', flow_a.data_ptr(), flow_b.data_ptr(), n, h, w, y0, x0, ch, cw, out.data_ptr())
    return out


TOF_CHUNK_BYTES = 256 << 20     # bound of one flow call's workspace + result in tof()


def tof(true_hwc, pred_hwc, window=None):
    """tOF of two (t, h, w, 3) uint8 device sequences: per consecutive pair, the mean end-point error between the
    Farneback flow of the true frames and that of the predicted ones, both computed on the frames cropped at the
    top left to the smaller of the two sizes; window = (y0, x0, h, w) of the flows enters the mean (None: all;
    the official protocol passes crop_8x8's).  -> float64 (t-1,) on the device.  Flows are computed in chunks of
    frames that overlap by one, so memory stays bounded; no value depends on the chunking."""
    _chk_u8(true_hwc, 'true'); _chk_u8(pred_hwc, 'pred')
    if true_hwc.dim() != 4 or pred_hwc.dim() != 4 or true_hwc.shape[0] != pred_hwc.shape[0] or true_hwc.shape[0] < 2:
        raise L.TecoganHipError(f'tof: shapes {tuple(true_hwc.shape)} / {tuple(pred_hwc.shape)} (two frames at least)')
    t = true_hwc.shape[0]
    h, w = min(true_hwc.shape[1], pred_hwc.shape[1]), min(true_hwc.shape[2], pred_hwc.shape[2])
    per_pair = L.lib().tg_farneback_workspace_bytes(2, h, w) - L.lib().tg_farneback_workspace_bytes(1, h, w)
    if per_pair <= 0:
        raise L.TecoganHipError(f'tof: frames of {h}x{w} (at least 16x16)')
    step = max(1, min(t - 1, TOF_CHUNK_BYTES // (per_pair + h * w * 8)))
    out = []
    for f0 in range(0, t - 1, step):
        f1 = min(t, f0 + step + 1)
        out.append(flow_epe_mean(farneback_flow(true_hwc[f0:f1], (h, w)), farneback_flow(pred_hwc[f0:f1], (h, w)),
                                 window))
    return torch.cat(out)


# ---------------------------------------------------------------------------
# training-side wrappers (backward kernels, losses, optimiser)
# ---------------------------------------------------------------------------
def pack_conv3x3_dgrad(weight, ocb=None):
    """Pack a Conv2d weight (cout,cin,3,3) for its DATA gradient: a conv3x3 op
    mapping cout -> cin with 180-degree rotated taps.  Returns (packed, op_cin, op_cout, ocb)."""
    w = _chk(weight, 'weight').detach()
    cout, cin = w.shape[0], w.shape[1]
    ocb = ocb or pick_ocb(cin)
    nfl = L.lib().tg_conv3x3_packed_floats(cout, cin, ocb)
    out = torch.empty(nfl, dtype=torch.float32, device=w.device)
    _call('tg_conv3x3_pack', w.data_ptr(), out.data_ptr(), cout, cin, ocb, 2)
    return out, cout, cin, ocb


def wgrad3x3(p, q, grad, cb_off=0, accumulate=True, bias_grad=None):
    """grad[a, cb_off:cb_off+cb, ky, kx] (+)= sum p[n,a,y,x] * q[n,b,y+ky-1,x+kx-1];
    bias_grad (ca,) (+)= sum of p (same launch, tg_wgrad3x3_multi_bias)."""
    if bias_grad is not None:
        return wgrad3x3_multi([p], [q], grad, cb_off=cb_off, accumulate=accumulate, bias_grad=bias_grad)
    _chk_all(p=p, q=q, grad=grad)
    n, ca, h, w = p.shape
    cb = q.shape[1]
    cb_total = grad.shape[1]
    if q.shape[0] != n or q.shape[2:] != p.shape[2:] or grad.shape[0] != ca or grad.shape[2:] != (3, 3):
        raise L.TecoganHipError(f'wgrad3x3: p {tuple(p.shape)} q {tuple(q.shape)} grad {tuple(grad.shape)}')
    ws = _workspace(4 * L.lib().tg_wgrad3x3_workspace_floats(n, ca, cb_total, h, w), p.device, cached=True)
    _call('tg_wgrad3x3', p.data_ptr(), ca * h * w, q.data_ptr(), cb * h * w, grad.data_ptr(), ws.data_ptr(), n, ca, cb,
          cb_total, cb_off, h, w, 1 if accumulate else 0)
    return grad


MAX_SEGS = 64


def _ptr_array(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _segments(accumulate, *lists):
    """The lists of segments one launch reads, MAX_SEGS at a time: yields (accumulate flag of the launch, a slice of
    each list).  Every launch behind the first adds to what the first one wrote."""
    for i in range(0, len(lists[0]), MAX_SEGS):
        yield (1 if (accumulate or i > 0) else 0, *(seg[i:i + MAX_SEGS] for seg in lists))


def wgrad3x3_multi(p_list, q_list, grad, cb_off=0, accumulate=True, phased=None, bias_grad=None):
    """wgrad3x3 over the concatenation of equally shaped (p_i, q_i) pairs without concatenating
    them: one launch reads up to MAX_SEGS separately allocated segments.
    phased = (cphase, taps_phase0, taps_phase1): q is a space-to-depth embedded tensor; only the
    taps each sub-pixel phase owns are computed (tg_wgrad3x3_multi_phased)."""
    if len(p_list) != len(q_list) or not p_list:
        raise L.TecoganHipError('wgrad3x3_multi: empty or mismatched lists')
    _chk_list(list(p_list) + list(q_list), 'segment')
    _chk(grad, 'grad')
    _chk_opt(bias_grad=bias_grad)
    n, ca, h, w = p_list[0].shape
    cb = q_list[0].shape[1]
    cb_total = grad.shape[1]
    for p_, q_ in zip(p_list, q_list):
        if p_.shape != p_list[0].shape or q_.shape != q_list[0].shape or q_.shape[0] != n \
                or q_.shape[2:] != p_.shape[2:]:
            raise L.TecoganHipError('wgrad3x3_multi: segments must share one shape')
    if grad.shape[0] != ca or grad.shape[2:] != (3, 3):
        raise L.TecoganHipError(f'wgrad3x3_multi: grad {tuple(grad.shape)}')
    if phased is not None and (cb_off or cb != cb_total):
        raise L.TecoganHipError('wgrad3x3_multi: phased taps take the whole q tensor')
    for acc, ps, qs in _segments(accumulate, p_list, q_list):
        ws = _workspace(4 * L.lib().tg_wgrad3x3_workspace_floats(n * len(ps), ca, cb_total, h, w), grad.device, cached=True)
        lead = (_ptr_array(ps), _ptr_array(qs), len(ps), ca * h * w, cb * h * w, grad.data_ptr())
        if phased is not None:
            _call('tg_wgrad3x3_multi_phased', *lead, ws.data_ptr(), n, ca, cb, h, w, acc, int(phased[0]), int(phased[1]),
                  int(phased[2]))
        elif bias_grad is not None:       # the layer's bias gradient out of the same pass over p = dZ
            _call('tg_wgrad3x3_multi_bias', *lead, bias_grad.data_ptr(), ws.data_ptr(), n, ca, cb, cb_total, cb_off, h, w,
                  acc)
        else:
            _call('tg_wgrad3x3_multi', *lead, ws.data_ptr(), n, ca, cb, cb_total, cb_off, h, w, acc)
    return grad


def wgrad3x3_convt_multi(x_list, dz_list, grad, accumulate=True, bias_grad=None):
    """tg_wgrad3x3_convt_multi: grad (ci, co, 3, 3) (+)= dW of ConvTranspose2d(ci, co, 3, 2, 1, 1) over the
    (input x_i (n, ci, h, w), output gradient dz_i (n, co, 2h, 2w)) pairs, straight from dZ; bias_grad (co,)
    (+)= the sum of dZ (same launch)."""
    if len(x_list) != len(dz_list) or not x_list:
        raise L.TecoganHipError('wgrad3x3_convt_multi: empty or mismatched lists')
    _chk_list(list(x_list) + list(dz_list), 'segment')
    _chk(grad, 'grad')
    _chk_opt(bias_grad=bias_grad)
    n, ci, h, w = x_list[0].shape
    co = dz_list[0].shape[1]
    if any(t.shape != x_list[0].shape for t in x_list) or any(t.shape != (n, co, 2 * h, 2 * w) for t in dz_list) \
            or tuple(grad.shape) != (ci, co, 3, 3):
        raise L.TecoganHipError(f'wgrad3x3_convt_multi: x {tuple(x_list[0].shape)} dz {tuple(dz_list[0].shape)} '
                                f'grad {tuple(grad.shape)}')
    for acc, xs, ds in _segments(accumulate, x_list, dz_list):
        ws = _workspace(4 * L.lib().tg_wgrad3x3_convt_workspace_floats(n * len(xs), ci, co, h, w), grad.device, cached=True)
        _call('tg_wgrad3x3_convt_multi', _ptr_array(xs), _ptr_array(ds), len(xs), grad.data_ptr(), _ptr(bias_grad),
              ws.data_ptr(), n, ci, co, h, w, acc)
    return grad


def wgrad3x3_body(dz_list, acts_list, grads, accumulate=True, dbs=None):
    """tg_wgrad3x3_body: weight gradients of the chained SRNet body's 2*nb residual-block convs over ALL
    unrolled frames in one launch.  dz_list[f] / acts_list[f]: (1 + 2nb, n, c, h, w) blocks of frame f
    (dz[2nb] = gradient of the body's output); grads: the 2nb weight-gradient tensors."""
    _chk_list(list(dz_list) + list(acts_list), 'block')
    _chk_list(grads, 'grad')
    _chk_list(dbs or (), 'dbs')
    nl, n, c, h, w = dz_list[0].shape
    if any(t.shape != dz_list[0].shape for t in list(dz_list) + list(acts_list)):
        raise L.TecoganHipError('wgrad3x3_body: frames must share one shape')
    if len(grads) != nl - 1 or len(dz_list) != len(acts_list):
        raise L.TecoganHipError('wgrad3x3_body: mismatched lists')
    for g in grads:
        if tuple(g.shape) != (c, c, 3, 3):
            raise L.TecoganHipError(f'wgrad3x3_body: grad {tuple(g.shape)}')
    for acc, dzs, acs in _segments(accumulate, dz_list, acts_list):
        ws = _workspace(4 * L.lib().tg_wgrad3x3_body_workspace_floats(len(dzs), n, nl - 1, c, h, w), grads[0].device,
                        cached=True)
        lead = (_ptr_array(dzs), _ptr_array(acs), len(dzs), n * c * h * w, nl - 1, _ptr_array(grads))
        if dbs is not None:         # dbs[L - 1] (+)= bias gradient of layer L = 1 .. 2nb, same launch
            _call('tg_wgrad3x3_body_bias', *lead, _ptr_array(dbs), ws.data_ptr(), n, c, h, w, acc)
        else:
            _call('tg_wgrad3x3_body', *lead, ws.data_ptr(), n, c, h, w, acc)


def bias_grad_body(dz_list, dbs):
    """tg_bias_grad_body: dbs[L] += bias gradient of layer L = 0 .. 2nb of the chained body, all frames."""
    _chk_list(list(dz_list) + list(dbs), 'tensor')
    nl, n, c, h, w = dz_list[0].shape
    if len(dbs) != nl:
        raise L.TecoganHipError('bias_grad_body: mismatched lists')
    for _, dzs in _segments(True, dz_list):         # (the entry point always adds)
        _call('tg_bias_grad_body', _ptr_array(dzs), len(dzs), n * c * h * w, nl, _ptr_array(dbs), n, c, h * w)


def bias_grad_multi(dy_list, db, accumulate=True):
    if not dy_list:
        raise L.TecoganHipError('bias_grad_multi: empty list')
    _chk_list(dy_list, 'segment')
    _chk(db, 'db')
    if any(t.shape != dy_list[0].shape for t in dy_list):
        raise L.TecoganHipError('bias_grad_multi: segments must share one shape')
    n, c = dy_list[0].shape[:2]
    hw = dy_list[0].numel() // (n * c)
    for acc, seg in _segments(accumulate, dy_list):
        _call('tg_bias_grad_multi', _ptr_array(seg), len(seg), db.data_ptr(), n, c, hw, acc)
    return db


def act_bwd(dy, y, act, out=None):
    _chk_all(dy=dy, y=y)
    out = _out(out, dy.shape, dy, 'act_bwd')
    _call('tg_act_bwd', dy.data_ptr(), y.data_ptr(), out.data_ptr(), dy.numel(), act)
    return out


def bias_grad(dy, db, accumulate=True):
    _chk_all(dy=dy, db=db)
    n, c = dy.shape[:2]
    hw = dy.numel() // (n * c)
    _call('tg_bias_grad', dy.data_ptr(), db.data_ptr(), n, c, hw, 1 if accumulate else 0)
    return db


def maxpool2_bwd(x, dy):
    _chk_all(x=x, dy=dy)
    n, c, h, w = x.shape
    dx = torch.empty_like(x)
    _call('tg_maxpool2_bwd', x.data_ptr(), dy.data_ptr(), dx.data_ptr(), n * c, h, w)
    return dx


def upsample_bwd(dy, scale, up_mode, mul=1.0):
    _chk(dy, 'dy')
    n, c, oh, ow = dy.shape
    h, w = oh // scale, ow // scale
    dx = torch.empty(n, c, h, w, dtype=torch.float32, device=dy.device)
    _call('tg_upsample_bwd', dy.data_ptr(), dx.data_ptr(), n * c, h, w, scale, up_mode, float(mul))
    return dx


def backward_warp_bwd(x, flow, dy, need_img=True, need_flow=True, dflow_out=None, dimg_acc=None, s2d=1):
    """`dflow_out`: write the flow gradient into this (contiguous, flow-shaped) buffer instead
    of a new tensor (a slice of the frame-major gradient of the training unroll).  `dimg_acc`: ADD the
    image gradient to this tensor (the gradient x already has) instead of returning a new one.
    `s2d` > 1: dy is the gradient of backward_warp_s2d's output (space_to_depth layout)."""
    _chk_all(x=x, flow=flow, dy=dy)
    n, c, h, w = x.shape
    if s2d > 1 and dy.shape != (n, s2d * s2d * c, h // s2d, w // s2d):
        raise L.TecoganHipError(f'backward_warp_bwd: dy {tuple(dy.shape)} vs x {tuple(x.shape)}, s2d {s2d}')
    acc = dimg_acc is not None
    dimg = _out(dimg_acc, x.shape, x, 'backward_warp_bwd', name='dimg_acc') if (acc or need_img) else None
    dflow = _out(dflow_out, flow.shape, flow, 'backward_warp_bwd', name='dflow_out') if need_flow else None
    lead = (x.data_ptr(), flow.data_ptr(), dy.data_ptr())
    if s2d > 1:
        _call('tg_backward_warp_s2d_bwd', *lead, _ptr(dimg), 1 if acc else 0, _ptr(dflow), n, c, h, w, s2d)
    elif acc:
        _call('tg_backward_warp_bwd_acc', *lead, dimg.data_ptr(), _ptr(dflow), n, c, h, w)
    else:
        _call('tg_backward_warp_bwd', *lead, _ptr(dimg), _ptr(dflow), n, c, h, w)
    return dimg, dflow


def depth_to_space(x, scale, act_y=None, act=ACT_NONE):
    """act_y / act: the result is the gradient of the activation output act_y and leaves multiplied by
    act'(.) (tg_depth_to_space_act_bwd); returns (y, fused) then."""
    _chk(x, 'x')
    _chk_opt(act_y=act_y)
    n, cs, h, w = x.shape
    c = cs // (scale * scale)
    y = torch.empty(n, c, h * scale, w * scale, dtype=torch.float32, device=x.device)
    fused = act_y is not None and act in (ACT_RELU, ACT_LRELU02) and act_y.shape == y.shape and bool(
        L.lib().tg_depth_to_space_act_bwd_supported(x.data_ptr(), act_y.data_ptr(), y.data_ptr(), w, scale))
    if fused:
        _call('tg_depth_to_space_act_bwd', x.data_ptr(), act_y.data_ptr(), act, y.data_ptr(), n, c, h, w, scale)
    else:
        _call('tg_depth_to_space', x.data_ptr(), y.data_ptr(), n, c, h, w, scale)
    return y if act_y is None else (y, fused)


def conv4x4s2_supported(n, ci, co, h, w):
    return bool(L.lib().tg_conv4x4s2_supported(n, ci, co, h, w))


def pack_conv4x4s2(w):
    """OIHW (co, ci, 4, 4) -> (forward pack, data-gradient pack) of tg_conv4x4s2_fwd / _dgrad."""
    _chk(w, 'w')
    co, ci = w.shape[:2]
    nfl = L.lib().tg_conv4x4s2_packed_floats(ci, co)
    pf = torch.empty(nfl, dtype=torch.float32, device=w.device)
    pd = torch.empty(nfl, dtype=torch.float32, device=w.device)
    _call('tg_conv4x4s2_pack', w.data_ptr(), pf.data_ptr(), pd.data_ptr(), ci, co)
    return pf, pd


def conv4x4s2(x, w_fwd, co, out=None):
    """nn.Conv2d(ci, co, 4, 2, 1, bias=False)(x) (tecogan_nets.py:322-340) on the direct kernel."""
    _chk_all(x=x, w_fwd=w_fwd)
    n, ci, h, w = x.shape
    y = _out(out, (n, co, h // 2, w // 2), x, 'conv4x4s2')
    # partial sums of the small-map form (no bytes: a null pointer)
    ws = _workspace(4 * L.lib().tg_conv4x4s2_workspace_floats(n, ci, co, h, w, 0), x.device)
    _call('tg_conv4x4s2_fwd', x.data_ptr(), w_fwd.data_ptr(), y.data_ptr(), ws.data_ptr() or None, n, ci, co, h, w)
    return y


def conv4x4s2_dgrad(g, w_dgrad, ci, act_y=None, act=ACT_NONE):
    """Gradient of conv4x4s2's input from the gradient g of its output; act_y / act: multiplied by act'(act_y)
    on the way out (act_y = the conv's input when that is an activation output)."""
    _chk_all(g=g, w_dgrad=w_dgrad)
    _chk_opt(act_y=act_y)
    n, co, oh, ow = g.shape
    if act_y is not None and act_y.shape != (n, ci, 2 * oh, 2 * ow):
        raise L.TecoganHipError(f'conv4x4s2_dgrad: act_y {tuple(act_y.shape)} vs g {tuple(g.shape)}, ci {ci}')
    dx = torch.empty(n, ci, 2 * oh, 2 * ow, dtype=torch.float32, device=g.device)
    ws = _workspace(4 * L.lib().tg_conv4x4s2_workspace_floats(n, ci, co, 2 * oh, 2 * ow, 1), g.device)
    _call('tg_conv4x4s2_dgrad', g.data_ptr(), w_dgrad.data_ptr(), _ptr(act_y), act, dx.data_ptr(), ws.data_ptr() or None,
          n, ci, co, 2 * oh, 2 * ow)
    return dx


def charbonnier(x, y, loss_accum, loss_scale, grad_scale=None, eps=1e-6):
    """loss_accum[0] += loss_scale * sum sqrt((x-y)^2+eps); returns d loss / dx (scaled) or None."""
    _chk_all(x=x, y=y)
    _chk_opt(loss_accum=loss_accum)
    dx = torch.empty_like(x) if grad_scale is not None else None
    _call('tg_charbonnier', x.data_ptr(), y.data_ptr(), x.numel(), float(eps), float(loss_scale), _ptr(loss_accum),
          float(grad_scale or 0.0), _ptr(dx))
    return dx


LOSS_L1, LOSS_MSE = L.TG_LOSS_L1, L.TG_LOSS_MSE


def pixel_loss(x, y, mode, loss_accum, loss_scale, grad_scale=None):
    """L1 / MSE: loss_accum[0] += loss_scale * sum v(x-y); returns scaled d loss / dx or None."""
    _chk_all(x=x, y=y)
    _chk_opt(loss_accum=loss_accum)
    if x.shape != y.shape:
        raise L.TecoganHipError(f'pixel_loss: {tuple(x.shape)} vs {tuple(y.shape)}')
    dx = torch.empty_like(x) if grad_scale is not None else None
    _call('tg_pixel_loss', x.data_ptr(), y.data_ptr(), x.numel(), int(mode), float(loss_scale), _ptr(loss_accum),
          float(grad_scale or 0.0), _ptr(dx))
    return dx


def channel_norm(x, mean, std):
    """(x - mean[c]) / std[c] over (n,c,h,w); mean None = 0."""
    _chk_all(x=x, std=std)
    _chk_opt(mean=mean)
    n, c, h, w = x.shape
    y = torch.empty_like(x)
    _call('tg_channel_norm', x.data_ptr(), _ptr(mean), std.data_ptr(), y.data_ptr(), n, c, h * w)
    return y


def cosine_loss(a, b, loss_accum, loss_scale, grad_scale=None, eps=1e-8):
    """loss_accum[0] += loss_scale * sum_pixels (1 - cos_c(a, b)); returns the scaled gradient
    w.r.t. a or None."""
    _chk_all(a=a, b=b)
    _chk_opt(loss_accum=loss_accum)
    if a.shape != b.shape:
        raise L.TecoganHipError(f'cosine_loss: {tuple(a.shape)} vs {tuple(b.shape)}')
    n, c, h, w = a.shape
    da = torch.empty_like(a) if grad_scale is not None else None
    _call('tg_cosine_loss', a.data_ptr(), b.data_ptr(), n, c, h * w, float(eps), float(loss_scale), _ptr(loss_accum),
          float(grad_scale or 0.0), _ptr(da))
    return da


def bce_logits(x, target, stats3, scale, grad_scale=None, dx_out=None, lsgan=False):
    """VanillaGANLoss (BCE with logits) or, lsgan=True, LSGANLoss (MSE) against a constant target."""
    _chk(x, 'x')
    _chk_opt(stats3=stats3)
    dx = _out(dx_out, x.shape, x, 'bce_logits', name='dx_out') if grad_scale is not None else None
    _call('tg_lsgan_loss' if lsgan else 'tg_bce_logits', x.data_ptr(), x.numel(), float(target), float(scale),
          _ptr(stats3), float(grad_scale or 0.0), _ptr(dx))
    return dx


def adam_step(p, g, m, v, lr, betas, eps, weight_decay, step, skip=None):
    """torch.optim.Adam step in place; `skip`: a device float -- non-zero turns the step into a no-op
    (the fault slot of the flat gradient buffer, see tg_adam_step_guarded)."""
    _chk_all(p=p, g=g, m=m, v=v)
    _chk_opt(skip=skip)
    args = (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), float(lr), float(betas[0]),
            float(betas[1]), float(eps), float(weight_decay), int(step))
    if skip is not None:
        _call('tg_adam_step_guarded', *args, skip.data_ptr())
    else:
        _call('tg_adam_step', *args)


def fault_to_slot(err_pinned, slot):
    """slot += 1 if the pinned int32 fault counter is non-zero (one thread; device-side read of host memory).
    err_pinned is the one operand of this module that is host memory by design: int32 and pinned, not on the device."""
    if not (torch.is_tensor(err_pinned) and err_pinned.dtype == torch.int32 and err_pinned.is_contiguous()
            and not err_pinned.is_cuda and err_pinned.is_pinned()):
        raise L.TecoganHipError('fault_to_slot: err_pinned: expected a pinned host int32 tensor')
    _chk(slot, 'slot')
    _call('tg_fault_to_slot', err_pinned.data_ptr(), slot.data_ptr())


def axpy_(y, x, a=1.0):
    _chk_all(y=y, x=x)
    _call('tg_axpy', y.data_ptr(), x.data_ptr(), float(a), y.numel())
    return y


def div_scalar_(y, d, x=None):
    """y = (x or y) / d, elementwise IEEE division."""
    _chk(y, 'y')
    src = y if x is None else _chk(x, 'x')
    _call('tg_div_scalar', y.data_ptr(), src.data_ptr(), float(d), y.numel())
    return y


def bn_lrelu_train_fwd(x, gamma, beta, running_mean, running_var, momentum=0.1, eps=1e-5, slope=0.2, out=None):
    _chk_all(x=x, gamma=gamma, beta=beta)
    _chk_opt(running_mean=running_mean, running_var=running_var)
    n, c, h, w = x.shape
    y = _out(out, x.shape, x, 'bn_lrelu_train_fwd')
    mean = torch.empty(c, dtype=torch.float32, device=x.device)
    invstd = torch.empty(c, dtype=torch.float32, device=x.device)
    _call('tg_bn_lrelu_train_fwd', x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), _ptr(running_mean),
          _ptr(running_var), float(momentum), float(eps), float(slope), y.data_ptr(), mean.data_ptr(), invstd.data_ptr(),
          n, c, h * w)
    return y, mean, invstd


def bn_lrelu_train_bwd(x, y, dy, gamma, mean, invstd, dgamma=None, dbeta=None, need_dx=True,
                       slope=0.2, dx_out=None):
    _chk_all(x=x, y=y, dy=dy, gamma=gamma, mean=mean, invstd=invstd)
    _chk_opt(dgamma=dgamma, dbeta=dbeta)
    n, c, h, w = x.shape
    dx = _out(dx_out, x.shape, x, 'bn_lrelu_train_bwd', name='dx_out') if need_dx else None
    scratch = torch.empty(2 * c, dtype=torch.float32, device=x.device)
    _call('tg_bn_lrelu_train_bwd', x.data_ptr(), y.data_ptr(), dy.data_ptr(), gamma.data_ptr(), mean.data_ptr(),
          invstd.data_ptr(), float(slope), _ptr(dx), _ptr(dgamma), _ptr(dbeta), 1, scratch.data_ptr(), n, c, h * w)
    return dx


def linear1_fwd(x, w, b):
    _chk_all(x=x, w=w)
    _chk_opt(b=b)
    rows, k = x.shape
    y = torch.empty(rows, 1, dtype=torch.float32, device=x.device)
    _call('tg_linear1_fwd', x.data_ptr(), w.data_ptr(), _ptr(b), y.data_ptr(), rows, k)
    return y


def linear1_bwd(x, w, dy, dw=None, db=None, need_dx=True):
    _chk_all(x=x, w=w, dy=dy)
    _chk_opt(dw=dw, db=db)
    rows, k = x.shape
    dx = torch.empty_like(x) if need_dx else None
    _call('tg_linear1_bwd', x.data_ptr(), w.data_ptr(), dy.data_ptr(), _ptr(dx), _ptr(dw), _ptr(db), rows, k, 1)
    return dx


_BD_KERNELS = {}


def downsample_bd(x, kernel2d, scale, pad):
    """x (n,c,h,w) -> blurred + decimated (n,c,oh,ow); kernel2d: numpy (k,k) float32."""
    _chk(x, 'x')
    n, c, h, w = x.shape
    ks = int(kernel2d.shape[0])
    key = (str(x.device), ks, float(kernel2d[ks // 2, ks // 2]))
    kd = _BD_KERNELS.get(key)
    if kd is None:
        kd = _BD_KERNELS[key] = torch.from_numpy(kernel2d.copy()).to(x.device).contiguous()
    oh = (h - 1) // scale + 1 if pad else (h - ks) // scale + 1
    ow = (w - 1) // scale + 1 if pad else (w - ks) // scale + 1
    y = torch.empty(n, c, oh, ow, dtype=torch.float32, device=x.device)
    _call('tg_downsample_bd', x.data_ptr(), kd.data_ptr(), y.data_ptr(), n * c, h, w, ks, scale, 1 if pad else 0)
    return y


BI_TILE = (L.TG_BI_TILE_H, L.TG_BI_TILE_W)      # LR pixels one workgroup of tg_downsample_bi_* makes
BI_BORDER_LR = 2         # pad=False: LR pixels cut from every side (= 2 * scale GT pixels of border)


def downsample_bi(x, scale, pad=True, out='f32'):
    """The BI degradation (generate_lr_bi.m: modcrop + imresize(1 / scale, 'bicubic') + 8-bit write) in exact integers,
    one launch (tg_downsample_bi_*).  x: uint8 (n,H,W,3) frames, or fp32 (n,3,H,W) in [0,1]
    whose values are first taken to their bytes (exact for the k / 255 every loader delivers).  scale 2 or 4.
    pad=True: LR (H // scale, W // scale), mirrored borders; pad=False: x carries 2 * scale pixels of border per side,
    LR is 4 smaller per axis.  out: 'f32' -> (n,3,h,w) fp32 = byte / 255, 'u8' -> (n,h,w,3) uint8, 'both' -> (f32, u8)."""
    if not (torch.is_tensor(x) and x.is_cuda):
        raise L.TecoganHipError('downsample_bi: expected a CUDA/HIP tensor (no CPU path exists)')
    if out not in ('f32', 'u8', 'both'):
        raise L.TecoganHipError(f"downsample_bi: out is 'f32', 'u8' or 'both', got {out!r}")
    if x.dtype == torch.uint8 and x.dim() == 4 and x.shape[3] == 3:
        _chk_u8(x, 'x')
        n, h, w, _ = x.shape
        name = 'tg_downsample_bi_u8'
    elif x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == 3:
        _chk(x, 'x')
        n, _, h, w = x.shape
        name = 'tg_downsample_bi_f32'
    else:
        raise L.TecoganHipError(f'downsample_bi: expected uint8 (n,H,W,3) or fp32 (n,3,H,W), got {x.dtype} '
                                f'{tuple(x.shape)}')
    scale = int(scale)
    cut = 0 if pad else 2 * BI_BORDER_LR
    oh, ow = max(h // max(scale, 1) - cut, 0), max(w // max(scale, 1) - cut, 0)    # the library refuses what is empty
    y32 = torch.empty(n, 3, oh, ow, dtype=torch.float32, device=x.device) if out != 'u8' else None
    y8 = torch.empty(n, oh, ow, 3, dtype=torch.uint8, device=x.device) if out != 'f32' else None
    _call(name, x.data_ptr(), _ptr(y8), _ptr(y32), n, h, w, scale, 1 if pad else 0)
    return y32 if out == 'f32' else (y8 if out == 'u8' else (y32, y8))


# ---- bicubic resize to any size ----
RESAMPLE_MAX_TAPS, RESAMPLE_WEIGHT_BITS = L.TG_RESAMPLE_MAX_TAPS, L.TG_RESAMPLE_WEIGHT_BITS
_RESAMPLE_DEVICE_TABLES = {}                     # (n_in, n_out, device) -> (idx, w) on the device
_RESAMPLE_CACHE_ENTRIES = 64


def resample_ratio_ok(n_in, n_out):
    """Whether tg_resample_u8 takes n_in -> n_out along an axis: both >= 1, n_out / n_in in [1/4, 4]."""
    return n_in >= 1 and n_out >= 1 and 4 * n_out >= n_in and n_out <= 4 * n_in


def _cubic(x):
    ax = np.abs(x)
    ax2, ax3 = ax * ax, ax * ax * ax
    return (1.5 * ax3 - 2.5 * ax2 + 1) * (ax <= 1) + (-0.5 * ax3 + 2.5 * ax2 - 4 * ax + 2) * ((1 < ax) & (ax <= 2))


def resample_tables(n_in, n_out):
    """The tables tg_resample_u8 takes for one axis, numpy (idx int32 (n_out, P), w int16 (n_out, P)): MATLAB
    imresize's contributions() for 'bicubic' in fp64 -- cubic kernel a = -0.5, stretched by n_in / n_out when
    shrinking, weights normalised, indices mirrored with the edge pixel repeated, all-zero columns dropped -- then
    w = rint(weight * 2^14) with the row's residual 2^14 - sum(w) added to its largest entry (the first on a tie), so
    every row sums to exactly 2^14.  tests/resize_ref.py is the specification; the arithmetic here is the same, in the
    same order."""
    n_in, n_out = int(n_in), int(n_out)
    if not resample_ratio_ok(n_in, n_out):
        raise L.TecoganHipError(f'resample_tables: {n_in} -> {n_out}: both sizes are >= 1 and the ratio lies in [1/4, 4]')
    scale = n_out / n_in
    kernel_width = 4.0
    if scale < 1:
        def h(x):
            return scale * _cubic(scale * x)
        kernel_width = kernel_width / scale
    else:
        h = _cubic
    x = np.arange(1, n_out + 1, dtype=np.float64)
    u = x / scale + 0.5 * (1 - 1 / scale)
    left = np.floor(u - kernel_width / 2)
    P = int(np.ceil(kernel_width)) + 2
    indices = left[:, None] + np.arange(P, dtype=np.float64)[None, :]
    weights = h(u[:, None] - indices)
    weights = weights / weights.sum(axis=1, keepdims=True)
    aux = np.concatenate([np.arange(1, n_in + 1), np.arange(n_in, 0, -1)])
    indices = aux[np.mod(indices.astype(np.int64) - 1, 2 * n_in)] - 1
    keep = np.any(weights != 0, axis=0)
    weights, indices = weights[:, keep], indices[:, keep]
    one = 1 << RESAMPLE_WEIGHT_BITS
    q = np.rint(weights * one).astype(np.int64)
    q[np.arange(n_out), np.argmax(q, axis=1)] += one - q.sum(axis=1)
    if q.shape[1] > RESAMPLE_MAX_TAPS or np.abs(q).max() >= 2 ** 15:
        raise L.TecoganHipError(f'resample_tables: {n_in} -> {n_out}: {q.shape[1]} taps, largest weight {np.abs(q).max()}')
    return np.ascontiguousarray(indices, dtype=np.int32), np.ascontiguousarray(q, dtype=np.int16)


def resample_tables_device(n_in, n_out, device):
    """resample_tables on `device`, as (idx, w, taps); cached per (n_in, n_out, device)."""
    device = torch.device(device)
    if device.index is None:
        device = torch.device('cuda', torch.cuda.current_device())
    key = (int(n_in), int(n_out), device)
    hit = _RESAMPLE_DEVICE_TABLES.get(key)
    if hit is None:
        idx, w = resample_tables(n_in, n_out)
        if len(_RESAMPLE_DEVICE_TABLES) >= _RESAMPLE_CACHE_ENTRIES:
            _RESAMPLE_DEVICE_TABLES.clear()
        hit = _RESAMPLE_DEVICE_TABLES[key] = (torch.from_numpy(idx).to(device), torch.from_numpy(w).to(device),
                                              idx.shape[1])
    return hit


def resize_u8(x, size, out=None):
    """(n,H,W,3) uint8 frames on device -> (n,h,w,3) uint8, size = (h, w): MATLAB-style antialiased bicubic in exact
    integers, one launch (tg_resample_u8), the bytes of tests/resize_ref.py.  Either ratio lies
    in [1/4, 4]; at 1/2 and 1/4 of a multiple of 2 or 4 the bytes are downsample_bi's.  out: a contiguous (n,h,w,3)
    uint8 tensor on x's device to write into."""
    if not (torch.is_tensor(x) and x.is_cuda):
        raise L.TecoganHipError('resize_u8: expected a CUDA/HIP tensor (no CPU path exists)')
    _chk_u8(x, 'x')
    if x.dim() != 4 or x.shape[3] != 3 or x.shape[0] < 1:
        raise L.TecoganHipError(f'resize_u8: expected uint8 (n,H,W,3) with n >= 1, got shape {tuple(x.shape)}')
    try:
        h, w = (int(v) for v in size)
    except (TypeError, ValueError):
        raise L.TecoganHipError(f'resize_u8: size is (h, w), got {size!r}') from None
    n, H, W, _ = x.shape
    if not (resample_ratio_ok(H, h) and resample_ratio_ok(W, w)):
        raise L.TecoganHipError(f'resize_u8: {H}x{W} -> {h}x{w}: the ratio of either axis lies in [1/4, 4]')
    out = _out(out, (n, h, w, 3), x, 'resize_u8', torch.uint8)
    vi, vw, vt = resample_tables_device(H, h, x.device)
    hi, hw, ht = resample_tables_device(W, w, x.device)
    _call('tg_resample_u8', _ptr(x), _ptr(out), n, H, W, h, w, _ptr(vi), _ptr(vw), vt, _ptr(hi), _ptr(hw), ht)
    return out


# ---- SyncBatchNorm (+LeakyReLU): statistics exchanged over ranks between the halves ----
def sync_bn_lrelu_train_fwd_groups(x, groups, gamma, beta, running_mean, running_var, momentum=0.1, eps=1e-5,
                                   slope=0.2):
    """bn_lrelu_train_fwd with statistics over the GLOBAL batch, for `groups` INDEPENDENT batches stacked along n (the
    critic's real and fake pass run as one pair batch, vsrgan_model.py:137-153).  Every rank computes (mean, centred M2)
    of its slice of each group, ONE all-gather of groups x 2c floats per layer, merged per group with Chan's formula in
    rank order (equal per-rank batch sizes, as DistributedSampler guarantees) -- the formulation torch's SyncBatchNorm
    uses, with no E[x^2] - mean^2 cancellation; running statistics updated group after group (the order of the
    reference's separate passes).  Returns y and per-group (mean, invstd, count).  With one rank the result is
    bit-identical to bn_lrelu_train_fwd."""
    from .utils import dist_utils
    _chk_all(x=x, gamma=gamma, beta=beta)
    _chk_opt(running_mean=running_mean, running_var=running_var)
    n, c, h, w = x.shape
    per = n // groups
    local = torch.empty(groups * 2 * c, dtype=torch.float32, device=x.device)
    for g in range(groups):
        _call('tg_bn_local_stats', x[g * per:(g + 1) * per].data_ptr(), local[g * 2 * c:].data_ptr(), per, c, h * w)
    gathered = dist_utils.all_gather_flat(local)                     # (world, groups * 2c)
    world = gathered.shape[0]
    count = float(per * h * w * world)
    y = torch.empty_like(x)
    stats = []
    for g in range(groups):
        part = gathered[:, g * 2 * c:(g + 1) * 2 * c].contiguous()
        mean = torch.empty(c, dtype=torch.float32, device=x.device)
        invstd = torch.empty(c, dtype=torch.float32, device=x.device)
        _call('tg_bn_merge_stats', part.data_ptr(), world, float(per * h * w), float(eps), float(momentum),
              mean.data_ptr(), invstd.data_ptr(), _ptr(running_mean), _ptr(running_var), c)
        _call('tg_bn_lrelu_apply', x[g * per:(g + 1) * per].data_ptr(), mean.data_ptr(), invstd.data_ptr(),
              gamma.data_ptr(), beta.data_ptr(), float(slope), y[g * per:(g + 1) * per].data_ptr(), per, c, h * w)
        stats.append((mean, invstd, count))
    return y, stats


def sync_bn_lrelu_train_bwd_groups(x, y, dy, groups, gamma, stats, dgamma=None, dbeta=None, need_dx=True, slope=0.2):
    """Backward of sync_bn_lrelu_train_fwd_groups: ONE all-reduce of the groups x 2c sums per layer.  dgamma/dbeta
    receive the LOCAL sums (DDP averages parameter gradients afterwards, as SyncBatchNorm does); dx uses the global
    sums."""
    from .utils import dist_utils
    _chk_all(x=x, y=y, dy=dy, gamma=gamma)
    _chk_opt(dgamma=dgamma, dbeta=dbeta)
    for st in stats:
        _chk_all(mean=st[0], invstd=st[1])
    n, c, h, w = x.shape
    per = n // groups
    sums = torch.empty(groups * 2 * c, dtype=torch.float32, device=x.device)
    for g in range(groups):
        sl = slice(g * per, (g + 1) * per)
        _call('tg_bn_lrelu_bwd_reduce', x[sl].data_ptr(), y[sl].data_ptr(), dy[sl].data_ptr(), stats[g][0].data_ptr(),
              stats[g][1].data_ptr(), float(slope), sums[g * 2 * c:].data_ptr(), per, c, h * w)
        if dgamma is not None:
            axpy_(dgamma, sums[g * 2 * c + c:(g + 1) * 2 * c], 1.0)
            axpy_(dbeta, sums[g * 2 * c:g * 2 * c + c], 1.0)
    dist_utils.all_reduce_sum_(sums)
    dx = None
    if need_dx:
        dx = torch.empty_like(x)
        for g in range(groups):
            sl = slice(g * per, (g + 1) * per)
            _call('tg_bn_lrelu_bwd_apply', x[sl].data_ptr(), y[sl].data_ptr(), dy[sl].data_ptr(), stats[g][0].data_ptr(),
                  stats[g][1].data_ptr(), gamma.data_ptr(), sums[g * 2 * c:].data_ptr(), float(slope), 1.0 / stats[g][2],
                  dx[sl].data_ptr(), per, c, h * w)
    return dx


def sync_bn_lrelu_train_fwd(x, gamma, beta, running_mean, running_var, momentum=0.1, eps=1e-5, slope=0.2):
    """One batch: the one-group case.  Returns (y, mean, invstd, count)."""
    y, stats = sync_bn_lrelu_train_fwd_groups(x, 1, gamma, beta, running_mean, running_var, momentum, eps, slope)
    return (y,) + stats[0]


def sync_bn_lrelu_train_bwd(x, y, dy, gamma, mean, invstd, count, dgamma=None, dbeta=None, need_dx=True, slope=0.2):
    return sync_bn_lrelu_train_bwd_groups(x, y, dy, 1, gamma, [(mean, invstd, count)], dgamma, dbeta, need_dx, slope)


# ---- data movement of the training step (tg_assemble.hip) ---------------------------------
def time_gather(x, idx):
    """x (n, t, ...) -> (n, len(idx), ...) with out[:, k] = x[:, idx[k]] (one launch)."""
    _chk(x, 'x')
    n, t = x.shape[:2]
    inner = x[0, 0].numel()
    out = torch.empty((n, len(idx)) + tuple(x.shape[2:]), dtype=torch.float32, device=x.device)
    arr = (ctypes.c_int * len(idx))(*[int(i) for i in idx])
    _call('tg_time_gather', x.data_ptr(), out.data_ptr(), arr, n, t, len(idx), inner)
    return out


def pingpong(x):
    """cat([x, x.flip(1)[:, 1:]], 1) (vsrgan_model.py:112-119)."""
    t = x.shape[1]
    return time_gather(x, list(range(t)) + list(range(t - 2, -1, -1)))


def pingpong_grad(g, te):
    """Ping-pong loss gradient g (n, te-1, ...) -> (n, 2*te-1, ...): +g | 0 | -flip(g)."""
    _chk(g, 'g')
    n = g.shape[0]
    inner = g[0, 0].numel()
    out = torch.empty((n, 2 * te - 1) + tuple(g.shape[2:]), dtype=torch.float32, device=g.device)
    _call('tg_pingpong_grad', g.data_ptr(), out.data_ptr(), n, te, inner)
    return out


def d_assemble_fwd(data, warped, cond, t, pad, crop, out=None):
    """Discriminator input (n*t/3, 9c, h, w) from data (n, T, c, h, w), warped (n*t, c, h, w),
    cond (n, T', c, h, w); `out`: a contiguous (n*t/3, 9c, h, w) destination (half of a pair batch)."""
    _chk_all(data=data, warped=warped, cond=cond)
    n, t_data, c, h, w = data.shape
    x = _out(out, (n * t // 3, 9 * c, h, w), data, 'd_assemble_fwd')
    _call('tg_d_assemble_fwd', data.data_ptr(), t_data, warped.data_ptr(), cond.data_ptr(), cond.shape[1], x.data_ptr(),
          n, t, c, h, w, pad, crop)
    return x


def d_assemble_bwd(g, n, t, t_data, c, pad, crop):
    """-> (g_data (n, t_data, c, h, w), g_warped (n*t, c, h, w))."""
    _chk(g, 'g')
    h, w = g.shape[2:]
    g_data = torch.empty(n, t_data, c, h, w, dtype=torch.float32, device=g.device)
    g_warped = torch.empty(n * t, c, h, w, dtype=torch.float32, device=g.device)
    _call('tg_d_assemble_bwd', g.data_ptr(), g_data.data_ptr(), t_data, g_warped.data_ptr(), n, t, c, h, w, pad, crop)
    return g_data, g_warped


def transpose01(x):
    """(a, b, ...) -> (b, a, ...) contiguous (clip-major <-> frame-major), one launch."""
    _chk(x, 'x')
    a, b = x.shape[:2]
    y = torch.empty((b, a) + tuple(x.shape[2:]), dtype=torch.float32, device=x.device)
    _call('tg_transpose01', x.data_ptr(), y.data_ptr(), a, b, x[0, 0].numel())
    return y


def stack_time(frames):
    """torch.stack(frames, dim=1) of k <= 64 contiguous (n, ...) tensors, one launch."""
    _chk_list(frames, 'frame')
    n = frames[0].shape[0]
    y = torch.empty((n, len(frames)) + tuple(frames[0].shape[1:]), dtype=torch.float32,
                    device=frames[0].device)
    _call('tg_stack_time', _ptr_array(frames), len(frames), y.data_ptr(), n, frames[0][0].numel())
    return y


def index_gather(src, idx, out=None, accumulate=False):
    """out.flat[i] (+)= src.flat[idx[i]] (0 where idx[i] is out of range); idx int64 on device."""
    _chk(src, 'src'); _chk(idx, 'idx', torch.int64)
    _chk_opt(out=out)
    if out is None and accumulate:
        raise L.TecoganHipError('index_gather: accumulate adds to a given out')
    if out is None:
        out = torch.empty(idx.numel(), dtype=torch.float32, device=src.device)
    elif out.numel() != idx.numel():
        raise L.TecoganHipError(f'index_gather: out {tuple(out.shape)} for idx {tuple(idx.shape)}')
    _call('tg_index_gather', src.data_ptr(), idx.data_ptr(), out.data_ptr(), idx.numel(), src.numel(), int(accumulate))
    return out


# ---- Winograd F(2x2, 3x3) form of conv3x3 (tg_conv3x3_wino.hip) ----------------------------
def pack_conv3x3_wino(w, transposed=0):
    """OIHW weights -> transformed, lane-ordered U (see tg_pack_conv3x3_wino)."""
    _chk(w, 'w')
    co, ci = (w.shape[0], w.shape[1]) if transposed == 0 else (w.shape[1], w.shape[0])
    nflt = L.lib().tg_conv3x3_wino_packed_floats(ci, co)
    out = torch.empty(nflt, dtype=torch.float32, device=w.device)
    _call('tg_pack_conv3x3_wino', w.data_ptr(), out.data_ptr(), ci, co, transposed)
    return out


WINO_POOL, WINO_UP2 = L.TG_WINO_POOL, L.TG_WINO_UP2


def _nstride(t):
    return 0 if t is None else t.stride(0)


def conv3x3_wino(x, u_packed, bias, cin, cout, act=ACT_NONE, x2=None, res=None, mask=None, out=None, pool=False,
                 up2=False):
    """tg_conv3x3_wino_fwd.  pool: MaxPool2d(2, 2) folded into the epilogue, the result is (n, cout, h/2, w/2);
    up2: x is the (n, cin, h/2, w/2) source of a bilinear x2 up-sampling folded into the input staging
    (tg_conv3x3_wino_fused_fwd: single source, no residual, no mask; bit-identical to the separate launches).
    res, mask and out go in with a batch stride of their own (_chk_batched); x and x2 are contiguous."""
    _chk_all(x=x, u_packed=u_packed)
    _chk_opt(bias=bias, x2=x2)
    for name, t in (('res', res), ('mask', mask)):
        if t is not None:
            _chk_batched(t, name)
    n, c1, h, w = x.shape
    if c1 + (0 if x2 is None else x2.shape[1]) != cin:
        raise L.TecoganHipError(f'conv3x3_wino: x {tuple(x.shape)}, x2 {None if x2 is None else tuple(x2.shape)}: '
                                f'the weights expect {cin} channels')
    if pool or up2:
        if x2 is not None or res is not None or mask is not None:
            raise L.TecoganHipError('conv3x3_wino: pool / up2 take a single source, no residual and no mask')
        if up2:
            h, w = 2 * h, 2 * w
        y = _out(out, (n, cout, h // 2 if pool else h, w // 2 if pool else w), x, 'conv3x3_wino', chk=_chk_batched)
        _call('tg_conv3x3_wino_fused_fwd', x.data_ptr(), x.stride(0), u_packed.data_ptr(), _ptr(bias), y.data_ptr(),
              y.stride(0), n, cin, cout, h, w, act, (WINO_POOL if pool else 0) | (WINO_UP2 if up2 else 0))
        return y
    y = _out(out, (n, cout, h, w), x, 'conv3x3_wino', chk=_chk_batched)
    _call('tg_conv3x3_wino_fwd', x.data_ptr(), x.stride(0), c1, _ptr(x2), _nstride(x2), u_packed.data_ptr(), _ptr(bias),
          _ptr(res), _nstride(res), _ptr(mask), _nstride(mask), y.data_ptr(), y.stride(0), n, cin, cout, h, w, act)
    return y


def pack_upconv(w, ocb=0, cin=None, cout=None):
    """tg_upconv_pack: the tap-GEMM operand of conv3x3(bilinear_x2(.)).  ocb 0: w is the OIHW weight; 32 | 64: w is
    pack_conv3x3's layout with that ocb (cin, cout then given)."""
    _chk(w, 'w')
    if ocb == 0:
        cout, cin = w.shape[0], w.shape[1]
    nflt = L.lib().tg_upconv_packed_floats(cin, cout)
    if nflt == 0:
        raise L.TecoganHipError(f'pack_upconv: cin={cin} cout={cout} is not a supported shape')
    out = torch.empty(nflt, dtype=torch.float32, device=w.device)
    _call('tg_upconv_pack', w.data_ptr(), out.data_ptr(), cin, cout, ocb)
    return out


def _upconv_x(x, a_packed, bias, cin, who):
    """The checks the three upconv wrappers share: x contiguous with cin channels, the packed operand, the bias."""
    _chk_all(x=x, a_packed=a_packed)
    _chk_opt(bias=bias)
    if x.shape[1] != cin:
        raise L.TecoganHipError(f'{who}: x {tuple(x.shape)}, the weights expect {cin} channels')
    return x.shape[0], x.shape[2], x.shape[3]


def upconv_tap_gemm(x, a_packed, cin, cout, z=None):
    """z (n, 9 cout, h, w) = the nine taps' channel mixes of x (n, cin, h, w) at its own resolution."""
    n, h, w = _upconv_x(x, a_packed, None, cin, 'upconv_tap_gemm')
    z = _out(z, (n, 9 * cout, h, w), x, 'upconv_tap_gemm', name='z', chk=_chk_batched)
    _call('tg_upconv_tap_gemm', x.data_ptr(), x.stride(0), a_packed.data_ptr(), z.data_ptr(), z.stride(0), n, cin, cout,
          h, w)
    return z


def upconv_combine(z, bias, cout, act=ACT_NONE, out=None):
    """y (n, cout, 2h, 2w) = act(bias + the nine shifted, bilinearly x2 up-sampled planes of z (n, 9 cout, h, w))."""
    _chk(z, 'z')
    _chk_opt(bias=bias)
    n, c9, h, w = z.shape
    if c9 != 9 * cout:
        raise L.TecoganHipError(f'upconv_combine: z {tuple(z.shape)} for {cout} output channels')
    y = _out(out, (n, cout, 2 * h, 2 * w), z, 'upconv_combine', chk=_chk_batched)
    _call('tg_upconv_combine', z.data_ptr(), z.stride(0), _ptr(bias), y.data_ptr(), y.stride(0), n, cout, h, w, act)
    return y


def upconv3x3(x, a_packed, bias, cin, cout, act=ACT_NONE, out=None):
    """act(conv3x3(bilinear_x2(x)) + bias) with the matrix work at x's resolution (tg_upconv3x3_fwd: both launches)."""
    n, h, w = _upconv_x(x, a_packed, bias, cin, 'upconv3x3')
    y = _out(out, (n, cout, 2 * h, 2 * w), x, 'upconv3x3', chk=_chk_batched)
    z = torch.empty(n, 9 * cout, h, w, dtype=torch.float32, device=x.device)
    _call('tg_upconv3x3_fwd', x.data_ptr(), x.stride(0), a_packed.data_ptr(), _ptr(bias), z.data_ptr(), z.stride(0),
          y.data_ptr(), y.stride(0), n, cin, cout, h, w, act)
    return y


def _fill_layer(a, d, packed, cin, cout=None):
    """One tg_chain_layer / tg_wino_layer (`a`) from a layer dict `d` (checked by _chk_layers) and its packed weights;
    cout: the chain layer's own (a wino chain has one for all layers), with it the mask, which only that struct has."""
    x, x2, res, y = d['x'], d.get('x2'), d.get('res'), d['y']
    a.x, a.x2, a.bias, a.res, a.y = x.data_ptr(), _ptr(x2), _ptr(d.get('bias')), _ptr(res), y.data_ptr()
    a.x_nstride, a.x2_nstride, a.res_nstride, a.y_nstride = x.stride(0), _nstride(x2), _nstride(res), y.stride(0)
    a.c1, a.cin, a.act = x.shape[1], cin, d.get('act', ACT_NONE)
    if cout is None:
        a.u_packed = packed.data_ptr()
    else:
        mask = d.get('mask')
        a.w_packed, a.cout, a.relu_mask, a.mask_nstride = packed.data_ptr(), cout, _ptr(mask), _nstride(mask)


class RowChain:
    """tg_conv3x3_chain: dependent 3x3 layers of small frames in one persistent launch.  `layers` is a
    list of dicts (x, w (OIHW weight tensor), bias=None, act=ACT_NONE, x2=None, res=None, mask=None, y);
    the weights are packed here in the layout the launcher's choice for this shape needs."""

    def __init__(self, layers, n, h, w):
        _chk_layers(layers, 'RowChain', 'w')
        lib = L.lib()
        self.n, self.h, self.w = n, h, w
        self.parts = lib.tg_conv3x3_chain_supported(n, h, w, 64)
        if self.parts == 0:
            raise L.TecoganHipError(f'RowChain: {n}x{h}x{w} cannot run as a chained launch on this device')
        self.layout = 16 if self.parts == 4 else 64
        self.keep = [layers]
        self.arr = (L.ChainLayer * len(layers))()
        for a, d in zip(self.arr, layers):
            wt = d['w']
            pk = pack_conv3x3_m16(wt) if self.layout == 16 else pack_conv3x3(wt, ocb=64)[0]
            self.keep.append(pk)
            _fill_layer(a, d, pk, wt.shape[1], wt.shape[0])
        self.nl = len(layers)
        self.flags = torch.zeros(lib.tg_conv3x3_chain_flag_ints(self.nl, n, h, w) + 16, dtype=torch.int32,
                                 device=layers[0]['x'].device)
        self.err = self.flags[-16:]
        self.epoch = 0

    def run(self, poll_limit=1 << 21):
        self.epoch += 1
        _call('tg_conv3x3_chain', self.arr, self.nl, self.n, self.h, self.w, self.layout, self.flags.data_ptr(),
              self.err.data_ptr(), self.epoch, poll_limit)

    def faults(self):
        return int(self.err[0].item())


class WinoChain:
    """tg_conv3x3_wino_chain: dependent 3x3 layers in one launch.  `layers` is a list of dicts
    (x, u, bias, cin, act, x2=None, res=None, y) of device tensors; the flag buffer and the epoch
    counter live here."""

    def __init__(self, layers, n, cout, h, w):
        _chk_layers(layers, type(self).__name__, 'u')
        self.n, self.cout, self.h, self.w = n, cout, h, w
        self.keep = layers
        self.arr = (L.WinoLayer * len(layers))()
        for a, d in zip(self.arr, layers):
            _fill_layer(a, d, d['u'], d['cin'])
        nints = L.lib().tg_conv3x3_wino_chain_flag_ints(len(layers), n, h, w)
        self.flags = torch.zeros(nints, dtype=torch.int32, device=layers[0]['x'].device)
        self.epoch = 0

    def run(self):
        self.epoch += 1
        _call('tg_conv3x3_wino_chain', self.arr, len(self.keep), self.n, self.cout, self.h, self.w,
              self.flags.data_ptr(), self.epoch)

    def bailouts(self):
        return int(self.flags[-16].item())


def pack_wres_convt(w):
    """nn.ConvTranspose2d(64, 64, 3, 2, 1, 1).weight (cin, cout, 3, 3) -> the A operands of the resident launch's
    transposed-conv tail (tg_conv3x3_wino_resident_ct_pack)."""
    _chk(w, 'w')
    if tuple(w.shape) != (64, 64, 3, 3):
        raise L.TecoganHipError(f'pack_wres_convt: weight {tuple(w.shape)}, expected (64, 64, 3, 3)')
    out = torch.empty(L.lib().tg_conv3x3_wino_resident_ct_floats(), dtype=torch.float32, device=w.device)
    _call('tg_conv3x3_wino_resident_ct_pack', w.data_ptr(), out.data_ptr())
    return out


class WinoResident(WinoChain):
    """tg_conv3x3_wino_resident: the same dependent layers of ONE frame on persistent, LDS-resident
    workgroups (tg_conv3x3_wino_res.hip).  Only layers[0]['x'] / ['x2'] are read and only
    layers[-1]['y'] is written."""

    def __init__(self, layers, cout, h, w):
        WinoChain.__init__(self, layers, 1, cout, h, w)
        nbytes = L.lib().tg_conv3x3_wino_resident_ws_bytes(h, w)
        self.ws = torch.zeros(nbytes // 4, dtype=torch.int32, device=layers[0]['x'].device)     # state, starts as zeros

    @staticmethod
    def supported(cout, h, w, n=1):
        return bool(L.lib().tg_conv3x3_wino_resident_supported(n, cout, h, w))

    def run(self, convt=None):
        """convt: None, or dict(u=pack_wres_convt(weight), bias=, y=(64, 2h, 2w) output, act=): SRNet's first
        ConvTranspose2d + act as the launch's tail (tg_conv3x3_wino_resident_ct); layers[-1]['y'] is then not written."""
        args = (self.arr, len(self.keep), self.cout, self.h, self.w, self.ws.data_ptr())
        if convt is None:
            self.epoch += 1
            _call('tg_conv3x3_wino_resident', *args, self.epoch)
            return
        _chk(convt['u'], 'WinoResident: convt u'); _chk(convt['bias'], 'WinoResident: convt bias')
        _chk_batched(convt['y'], 'WinoResident: convt y')
        self.epoch += 1
        ct = L.WresConvT(convt['u'].data_ptr(), convt['bias'].data_ptr(), convt['y'].data_ptr(), convt.get('act', ACT_RELU))
        _call('tg_conv3x3_wino_resident_ct', *args, self.epoch, ctypes.byref(ct))

    def bailouts(self):
        return int(self.ws[-64].item())


# ---- fp16 inference body of SRNet (tg_conv3x3_f16.hip) ---------------------------------
# fp16 tensors are torch.float16, activations channels-last (n, h, w, 64).

def f16_supported(n, cin, cout, h, w):
    return bool(L.lib().tg_conv3x3_f16_supported(int(n), int(cin), int(cout), int(h), int(w)))


def f16_pack_index(transposed=False, cin=64, cout=64):
    """Host statement of the packed fp16 weight order: an int64 array `idx` of tg_conv3x3_f16_packed_halves
    entries with packed[i] = weight.reshape(-1)[idx[i]] (or 0 where idx[i] < 0: channels padded to 64).
    Element ((ks * 4 + ct) * 64 + lane) * 8 + j is W[cout = 16 ct + lane % 16][tap = ks // 2]
    [cin = 32 (ks % 2) + 8 (lane // 16) + j] -- the A operand of v_mfma_f32_16x16x32_f16, K step ks."""
    i = np.arange(18 * 4 * 64 * 8, dtype=np.int64)
    j, lane, ct, ks = i & 7, (i >> 3) & 63, (i >> 9) & 3, i >> 11
    co, tap, ci = ct * 16 + (lane & 15), ks >> 1, (ks & 1) * 32 + (lane >> 4) * 8 + j
    src = ((ci * cout + co) if transposed else (co * cin + ci)) * 9 + tap
    return np.where((ci < cin) & (co < cout), src, -1)


def f16_pack_weights(w, transposed=False):
    """fp32 Conv2d (cout, cin, 3, 3) or ConvTranspose2d (cin, cout, 3, 3; transposed=True) weight -> packed fp16
    (round to nearest even), cin / cout <= 64 zero padded."""
    _chk(w, 'w')
    cin, cout = (w.shape[0], w.shape[1]) if transposed else (w.shape[1], w.shape[0])
    nh = L.lib().tg_conv3x3_f16_packed_halves(int(cin), int(cout))
    if nh == 0 or tuple(w.shape[2:]) != (3, 3):
        raise L.TecoganHipError(f'f16_pack_weights: weight {tuple(w.shape)} (3x3, at most 64 channels each way)')
    out = torch.empty(nh, dtype=torch.float16, device=w.device)
    _call('tg_conv3x3_f16_pack_weights', w.data_ptr(), int(cin), int(cout), 1 if transposed else 0, out.data_ptr())
    return out


def f16_pack_input(x1, x2=None):
    """fp32 NCHW x1 (and x2, concatenated behind it) -> fp16 channels-last (n, h, w, 64), zero padded."""
    _chk(x1, 'x1')
    _chk_opt(x2=x2)
    n, c1, h, w = x1.shape
    c2 = 0
    if x2 is not None:
        c2 = x2.shape[1]
        if (x2.shape[0], x2.shape[2], x2.shape[3]) != (n, h, w):
            raise L.TecoganHipError('f16_pack_input: x1 / x2 shapes differ')
    y = torch.empty(n, h, w, 64, dtype=torch.float16, device=x1.device)
    _call('tg_conv3x3_f16_pack_input', x1.data_ptr(), c1 * h * w, c1, _ptr(x2), c2 * h * w, c2, y.data_ptr(), n, h, w)
    return y


def conv3x3_f16(x, w_packed, bias, act=ACT_NONE, res=None, out=None):
    """x (n, h, w, 64) fp16 -> fp16: round16(act(conv3x3(x) + bias) + res).  out may be res, never x."""
    _chk_all(torch.float16, x=x, w_packed=w_packed)
    _chk(bias, 'bias')
    _chk_opt(torch.float16, res=res)
    n, h, w, c = x.shape
    if res is not None and res.shape != x.shape:
        raise L.TecoganHipError('conv3x3_f16: res shape differs from x')
    out = _out(out, x.shape, x, 'conv3x3_f16', torch.float16)
    _call('tg_conv3x3_f16_fwd', x.data_ptr(), w_packed.data_ptr(), bias.data_ptr(), _ptr(res), out.data_ptr(), n, c,
          bias.numel(), h, w, act)
    return out


def convt3x3s2_f16(x, w_packed, bias, act=ACT_NONE, out=None):
    """x (n, h, w, 64) fp16 -> fp32 NCHW (n, 64, 2h, 2w), not rounded: act(ConvTranspose2d(3, 2, 1, 1)(x) + bias)."""
    _chk_all(torch.float16, x=x, w_packed=w_packed)
    _chk(bias, 'bias')
    n, h, w, c = x.shape
    out = _out(out, (n, bias.numel(), 2 * h, 2 * w), x, 'convt3x3s2_f16')
    _call('tg_convt3x3s2_f16_fwd', x.data_ptr(), w_packed.data_ptr(), bias.data_ptr(), out.data_ptr(),
          bias.numel() * 4 * h * w, n, c, bias.numel(), h, w, act)
    return out
