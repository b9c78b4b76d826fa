"""One allocation for every operand of a launch, so that a kernel's stray read, stray write, unwritten output or ignored
batch stride shows instead of landing in memory that happens to be zero, free or already right.

`Arena` owns ONE tensor of 32-bit words on the device (or on the CPU, for tests/test_placement_cpu.py).  Operands are
carved out of it by `place` (a copy of a tensor) and `out` (a destination); every word no operand owns -- the margin in
front of, behind and between operands, and the gap between the images of an operand whose batch stride is not the
packed one -- holds a quiet NaN with a recognisable payload:

    GUARD | slot          GUARD = 0x7FC5A500, slot = 1, 2, ... the operand the word lies next to

(the NaN the hardware itself produces, 0x7FC00000 / 0xFFC00000, has an empty payload: a NaN a kernel computed can
never pass for an untouched guard, and the words are compared as int32, so NaN != NaN plays no part).  A destination
is pre-filled with its own slot's pattern.  The slot in the payload is what lets a failure NAME an operand: a NaN that
turns up in an output with the payload of slot k was READ from the guard words around operand k (0 * NaN is NaN: a
kernel that reads past a tensor and relies on a zero weight fails, which is intended -- in production the neighbour
holds anything); with the destination's own payload the element was never written.

Every operand has a margin of `margin_floats` words on both sides, and `place` / `out` refuse an operand larger than
the margin: a write at a wrong stride or one tile past the end still lands inside the arena.  That is what makes these
tests safe on a shared machine.

    a = Arena('cuda', margin_floats=4096)
    x = a.place(x_cpu, offset_floats=1, name='x')                 # base 4 bytes past a 64-byte boundary
    y = a.out((2, 48, 6, 8), nstride=48 * 48 + 8, name='y')       # 8 floats of gap between the two images
    rc = lib.tg_...(x.data_ptr(), a.nstride(x), ..., y.data_ptr(), a.nstride(y), ...)
    a.check()            # guards, gaps and inputs bit for bit as they were; names the nearest operand otherwise
    a.finite(y)          # every element written, no guard NaN leaked in

`inout` is the destination that already holds values (a gradient a launch adds to, or a gradient matrix of which a
launch writes a column slice): the elements outside the writable mask are checked like an input.
"""
import numpy as np
import torch

GUARD = 0x7FC5A500          # quiet NaN, payload 0x05A5xx: | slot (1..255)
ALIGN_WORDS = 16            # operand bases sit `offset_floats` past a 64-byte boundary


def pattern(slot):
    """The guard word of slot `slot` as a Python int that fits int32."""
    return GUARD | slot


def extent_floats(shape, nstride=None, itemsize=4):
    """32-bit words from the first to one past the last element of an operand of `shape` (images `nstride` ELEMENTS
    apart, default packed)."""
    n, per = _n_per(shape)
    ns = per if nstride is None else int(nstride)
    elems = (n - 1) * ns + per
    return (elems * itemsize + 3) // 4


def _n_per(shape):
    """(images, elements per image); a 1-D operand (bias, packed weights) is one image."""
    if len(shape) == 1:
        return 1, int(shape[0])
    return int(shape[0]), int(np.prod(shape[1:]))


class Arena:
    def __init__(self, device, margin_floats, slots=10, align_floats=ALIGN_WORDS):
        """align_floats: the largest alignment an operand of this arena asks of `out` (a multiple of ALIGN_WORDS; the
        default is what every operand gets)."""
        self.device = torch.device(device)
        self.margin = int(margin_floats)
        self.max_align = int(align_floats)
        assert self.max_align >= ALIGN_WORDS and self.max_align % ALIGN_WORDS == 0
        # each slot: margin | up to align_floats of alignment and 2 * ALIGN_WORDS of offset | operand (<= margin) | margin
        self.total = slots * (3 * self.margin + 3 * ALIGN_WORDS + self.max_align) + self.max_align
        if self.max_align == ALIGN_WORDS:
            self.words = torch.empty(self.total, dtype=torch.int32, device=self.device)
            assert self.words.data_ptr() % 64 == 0, 'the allocator returned a block that is not 64-byte aligned'
        else:       # the allocator promises no more: take the first word on the larger boundary
            raw = torch.empty(self.total + self.max_align, dtype=torch.int32, device=self.device)
            assert raw.data_ptr() % 4 == 0
            skip = (-(raw.data_ptr() // 4)) % self.max_align
            self.words = raw[skip:skip + self.total]
            assert self.words.data_ptr() % (4 * self.max_align) == 0
        self.words.fill_(pattern(0))               # words no slot has claimed yet (never next to an operand)
        self.expect = np.full(self.total, pattern(0), dtype=np.int32)      # what check() wants to find
        self.free = np.zeros(self.total, dtype=bool)                        # words a kernel may write
        self.ops = []                              # dicts: name, slot, base, words, per, ns, n, is_out
        self.cursor = 0
        self.max_slots = slots

    # ---- carving --------------------------------------------------------------------------------------------------
    def _carve(self, shape, dtype, offset_floats, nstride, name, is_out, align=ALIGN_WORDS):
        shape = tuple(int(s) for s in shape)
        itemsize = torch.empty(0, dtype=dtype).element_size()
        n, per = _n_per(shape)
        ns = per if nstride is None else int(nstride)
        assert nstride is None or len(shape) >= 2, 'a batch stride needs a batch dimension'
        assert ns >= per or n == 1, f'{name}: images would overlap (nstride {ns} < {per})'
        assert (per * itemsize) % 4 == 0 and (ns * itemsize) % 4 == 0, f'{name}: images must be whole 32-bit words'
        assert 0 <= offset_floats < 2 * ALIGN_WORDS
        words = extent_floats(shape, ns, itemsize)
        assert words <= self.margin, f'{name}: {words} words do not fit the margin of {self.margin}: a stray write ' \
                                     'of one operand extent could leave the arena'
        assert len(self.ops) < self.max_slots and len(self.ops) < 255, 'out of slots'
        slot = len(self.ops) + 1
        start = self.cursor
        assert ALIGN_WORDS <= align <= self.max_align and align % ALIGN_WORDS == 0, f'{name}: alignment {align}'
        base = (start + self.margin + align - 1) // align * align + int(offset_floats)
        end = base + words + self.margin
        assert end <= self.total
        self.cursor = end
        self.words[start:end] = pattern(slot)
        self.expect[start:end] = pattern(slot)
        op = dict(name=name or f'operand{slot}', slot=slot, base=base, words=words, n=n, is_out=is_out,
                  per_words=per * itemsize // 4, ns_words=ns * itemsize // 4, ns=ns)
        self.ops.append(op)
        flat = self.words.view(dtype)
        scale = 4 // itemsize
        inner = []
        acc = 1
        for s in reversed(shape[1:]):
            inner.append(acc)
            acc *= s
        strides = (ns,) + tuple(reversed(inner)) if len(shape) > 1 else (1,)
        assert len(shape) == 1 or tuple(reversed(inner))[-1] == 1
        view = torch.as_strided(flat, shape, strides, flat.storage_offset() + base * scale)
        view._arena_op = op
        return view, op

    def place(self, t, offset_floats=0, nstride=None, name=None):
        """A copy of `t` inside the arena: base `offset_floats` 32-bit words past a 64-byte boundary, images `nstride`
        elements apart (default packed), the gaps between images left as guard words.  Returns the view."""
        view, op = self._carve(t.shape, t.dtype, offset_floats, nstride, name, False)
        view.copy_(t)
        now = self.words[op['base']:op['base'] + op['words']].cpu().numpy()
        for b in range(op['n']):
            lo = b * op['ns_words']
            self.expect[op['base'] + lo:op['base'] + lo + op['per_words']] = now[lo:lo + op['per_words']]
        return view

    def out(self, shape, offset_floats=0, nstride=None, dtype=torch.float32, name='y', align_floats=ALIGN_WORDS, zero=False):
        """A destination of `shape`, pre-filled with its slot's guard pattern, placed as `place` does.  align_floats:
        the boundary the base is `offset_floats` past (a workspace that must be 256-byte aligned: 64).  zero: the
        images start as zeros instead (a flag buffer or workspace the entry point wants zeroed once); the gaps and
        margins keep the guard pattern."""
        view, op = self._carve(shape, dtype, offset_floats, nstride, name, True, align_floats)
        for b in range(op['n']):
            lo = op['base'] + b * op['ns_words']
            self.free[lo:lo + op['per_words']] = True
            if zero:
                self.words[lo:lo + op['per_words']] = 0
                self.expect[lo:lo + op['per_words']] = 0
        return view

    def inout(self, t, writable=None, prefill=False, offset_floats=0, nstride=None, name='g'):
        """A destination that already holds values (an accumulated gradient; a gradient matrix of which a launch
        writes a column slice): a copy of fp32 `t`, placed as `place` does, of which the launch may write the elements
        where the bool tensor `writable` (default: all) is set.  Every other element is checked bit for bit like an
        input.  prefill: the writable elements start as the slot's guard pattern instead of t's values (a launch that
        overwrites: finite() then tells an element that was never written)."""
        assert t.dtype == torch.float32
        view = self.place(t, offset_floats=offset_floats, nstride=nstride, name=name)
        op = view._arena_op
        op['is_out'] = True
        mask = torch.ones(t.shape, dtype=torch.bool) if writable is None else writable.expand(t.shape).contiguous()
        flat = mask.reshape(op['n'], -1).numpy()
        for b in range(op['n']):
            lo = op['base'] + b * op['ns_words']
            self.free[lo:lo + op['per_words']] = flat[b]
        if prefill:
            view.view(torch.int32)[mask.to(view.device)] = pattern(op['slot'])
            for b in range(op['n']):                 # (a refusal must leave the pre-fill as it is)
                lo = op['base'] + b * op['ns_words']
                self.expect[lo:lo + op['per_words']][flat[b]] = pattern(op['slot'])
        return view

    @staticmethod
    def nstride(view):
        """The batch stride of a view `place` / `out` returned, in elements: what the C ABI's `*_nstride` takes."""
        return view._arena_op['ns']

    # ---- checking -------------------------------------------------------------------------------------------------
    def _nearest(self, idx):
        best, where = None, None
        for op in self.ops:
            lo, hi = op['base'], op['base'] + op['words']
            d = 0 if lo <= idx < hi else (lo - idx if idx < lo else idx - hi + 1)
            if best is None or d < best[0]:
                if lo <= idx < hi:
                    b, r = divmod(idx - lo, op['ns_words'])
                    kind = 'gap behind image %d' % b if r >= op['per_words'] else 'image %d' % b
                    where = f"word {idx - lo:+d} from the base of {op['name']} ({kind}, {r - op['per_words']} words " \
                            f"past its end)" if r >= op['per_words'] else \
                            f"word {idx - lo:+d} from the base of {op['name']} ({kind})"
                elif idx < lo:
                    where = f"{lo - idx} words in front of {op['name']}"
                else:
                    where = f"{idx - hi + 1} words behind the end of {op['name']}"
                best = (d, op)
        return best[1], where

    def check(self, outputs_untouched=False):
        """Every word outside the destinations is bit for bit what it was: guard margins, gaps between images and the
        inputs themselves (a launch may not write a foreign operand).  outputs_untouched: the destinations still hold
        their pre-fill as well (a launcher that refused must not have launched)."""
        now = self.words.cpu().numpy()
        bad = now != self.expect
        if not outputs_untouched:
            bad &= ~self.free
        if bad.any():
            idx = np.flatnonzero(bad)
            op, where = self._nearest(int(idx[0]))
            raise AssertionError(
                f"arena: {idx.size} word(s) outside the destination changed; first: {where}: "
                f"0x{int(now[idx[0]]) & 0xFFFFFFFF:08X} (was 0x{int(self.expect[idx[0]]) & 0xFFFFFFFF:08X}); "
                f"nearest operand: {op['name']}")

    def finite(self, view):
        """Every element of destination `view` was written with a finite value.  On failure: whether the element still
        holds the pre-fill (never written), a guard word of another operand's surroundings (the kernel READ outside
        that operand), or a NaN / Inf of its own."""
        op = view._arena_op
        assert view.dtype in (torch.float32, torch.float16), 'finite() reads fp32 / fp16 destinations'
        v = view.detach().cpu().contiguous()
        fin = torch.isfinite(v)
        if bool(fin.all()):
            return
        bits = v.view(torch.int32).numpy().reshape(-1)           # (an image is whole words: halves pair up inside it)
        flat_bad = np.flatnonzero(~fin.numpy().reshape(-1))
        first = int(flat_bad[0])
        word = int(bits[first * v.element_size() // 4]) & 0xFFFFFFFF
        pos = tuple(int(p) for p in np.unravel_index(first, tuple(v.shape)))
        if (word & 0xFFFFFF00) == GUARD:
            slot = word & 0xFF
            if slot == op['slot']:
                why = f"{op['name']}{list(pos)} was never written (it still holds {op['name']}'s pre-fill)"
            else:
                src = next((o['name'] for o in self.ops if o['slot'] == slot), f'slot {slot}')
                why = f"{op['name']}{list(pos)} holds a guard word of {src}: the kernel read outside {src}"
        else:
            why = f"{op['name']}{list(pos)} = 0x{word:08X}: not finite, and not a guard word (a NaN whose payload was " \
                  "lost, or one the kernel computed)"
        raise AssertionError(f'arena: {flat_bad.size} element(s) of {op["name"]} are not finite; first: {why}')


# ---- the placements of tests/test_hip_placement.py (KERNELS.md, "Buffer placement") -------------------------------------
# name -> (offset_floats, extra floats on the packed batch stride, destination is a channel slice of a 3-channels-larger
# buffer)
PLACEMENTS = {
    'P0': (0, 0, False),      # aligned, packed
    'P1': (1, 0, False),      # base + 1 float: 4-byte aligned only
    'P2': (2, 0, False),      # base + 2 floats: 8-byte aligned (the Winograd form's float2 epilogue still allowed)
    'P3': (0, 1, False),      # aligned base, nstride = packed + 1: image 1 is 4-byte aligned only
    'P4': (0, 8, False),      # aligned base, nstride = packed + 8: 8 floats of gap that must survive
    'P5': (0, 0, True),       # destination = the first cout channels of a (n, cout + 3, h, w) buffer
}
