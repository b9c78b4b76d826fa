"""The kernels reach global memory through ONE buffer-access layer: the "raw buffer access" section of
csrc/tg_common.h (TG_BUF_RSRC, buf_ld, buf_st, BUF_OOB, BUF_SC1; KERNELS.md, "Buffer access").  A kernel source that
spells out the gfx950 builtins, the descriptor flags word, or a private copy of the out-of-range sentinel or of the
agent-scope cache-policy bit would make "is every cross-workgroup access sc1?" and "can this offset be mistaken for an
in-range one?" per-file questions again.  This reads the sources; nothing is compiled or launched."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'tecogan-pytorch_amd', 'csrc')
LAYER = 'tg_common.h'

# what only the layer may contain
FORBIDDEN = {
    'buffer load/store builtin': re.compile(r'__builtin_amdgcn_raw_buffer_'),
    'descriptor builtin': re.compile(r'__builtin_amdgcn_make_buffer_rsrc'),
    'descriptor flags literal': re.compile(r'\b0x0*20000\b', re.I),
    # `NAME_OOB = 0x80000000u` / `NAME_SC1 = 16` (also as a #define, in decimal or hex): a private sentinel / policy bit
    'private OOB / SC1 constant': re.compile(
        r'\b\w*(?:OOB|SC1)\b\s*(?:=|\s)\s*\(?\s*(?:0x80000000|2147483648|16|0x10)[uUlL]*\s*\)?\s*(?:;|,|$|//|/\*)', re.M),
}

# (file name, key of FORBIDDEN) -> why that file keeps the spelling.  A site goes here only when no spelling of the
# helpers reproduces its instructions (tools/isa_diff.sh); none does today.
ALLOWED = {}


def _sources():
    files = sorted(glob.glob(os.path.join(CSRC, '*.hip')) + glob.glob(os.path.join(CSRC, '*.h')))
    return {os.path.basename(f): open(f).read() for f in files}


def test_only_the_layer_spells_out_buffer_access():
    src = _sources()
    assert len(src) >= 20 and LAYER in src
    hits = {(name, what) for name, text in src.items() if name != LAYER
            for what, rx in FORBIDDEN.items() if rx.search(text)}
    unexpected = sorted(hits - set(ALLOWED))
    assert not unexpected, f'outside {LAYER}: {unexpected} -- use TG_BUF_RSRC / buf_ld / buf_st / BUF_OOB / BUF_SC1'
    stale = sorted(set(ALLOWED) - hits)
    assert not stale, f'allow-list entries no source needs any more: {stale}'
    assert all(isinstance(r, str) and r.strip() for r in ALLOWED.values()), 'every allow-list entry states its reason'


def test_the_layer_defines_each_piece_once():
    text = _sources()[LAYER]
    for what, rx in FORBIDDEN.items():
        assert rx.search(text), f'{LAYER} no longer holds the {what}'
    for decl in (r'constexpr unsigned BUF_OOB = 0x80000000u;', r'constexpr int BUF_SC1 = 16;',
                 r'constexpr int BUF_RSRC_FLAGS = 0x00020000;', r'#define TG_BUF_RSRC\(ptr, bytes\)',
                 r'\bT buf_ld\(__amdgpu_buffer_rsrc_t', r'\bvoid buf_st\(T v, __amdgpu_buffer_rsrc_t',
                 r'typedef float f32x2 ', r'typedef unsigned u32x2 ', r'typedef unsigned u32x4 '):
        assert len(re.findall(decl, text)) == 1, decl


def test_the_patterns_catch_what_they_are_for():
    """The per-file forms the kernels used to carry, and the packed sentinel that legitimately stays."""
    bad = ['constexpr unsigned RC_OOB = 0x80000000u;', '    constexpr unsigned OOB = 0x80000000u;   // >= any num_records',
           'constexpr int WR_SC1 = 16;     // agent scope', '#define MY_SC1 16', '#define X_OOB (0x80000000u)']
    for line in bad:
        assert FORBIDDEN['private OOB / SC1 constant'].search(line), line
    good = ['constexpr unsigned W_UP2_OOB = 0xFFFFFF80u;     // packed word', 'v = ok ? off : BUF_OOB;',
            'buf_st<BUF_SC1>(d, ry, yo);', 'constexpr int N_SC1 = 160;']
    for line in good:
        assert not FORBIDDEN['private OOB / SC1 constant'].search(line), line
    assert FORBIDDEN['descriptor flags literal'].search('rsrc(p, 0, n, 0x00020000)')
    assert FORBIDDEN['descriptor flags literal'].search('rsrc(p, 0, n, 0x20000)')
    assert not FORBIDDEN['descriptor flags literal'].search('0x00120000')
