"""ctypes binding of libtecogan_hip.so, derived from the C ABI's own header.

include/tecogan_hip.h is read once, at import, as text: its prototypes become SIGNATURES, its structs the
Structure classes, its enumerators and integer `#define TG_*` the module's TG_* constants.  An entry becomes
callable by declaring it there and rebuilding the library; nothing is restated here.  The header's leading
comment says what it may contain; anything else raises at import and names the declaration.

The library is built in-tree by `csrc/build.sh` (or __graft_entry__.build()).
Loading failures are loud: there is no fallback path.
"""
import collections
import ctypes as C
import math
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
# TECOGAN_HIP_LIB: measurement builds of the same sources (tools/build_var.sh, or csrc/build.sh with TG_LAB_BUILD=1); never a fallback
LIB_PATH = os.environ.get('TECOGAN_HIP_LIB') or os.path.join(_HERE, 'libtecogan_hip.so')
HEADER_PATH = os.path.join(os.path.dirname(_HERE), 'include', 'tecogan_hip.h')


class TecoganHipError(RuntimeError):
    pass


# The type rule, whole: these by value; `typedef void* NAME` handles by value, and every pointer or array
# parameter, as c_void_p (the pointee cannot tell device memory from a host out-parameter) -- except a single
# pointer to a struct whose fields the header declares: POINTER(that Structure).  Returns: the same, with
# `const char*` -> c_char_p and `void` -> None.
_SCALARS = {'int': C.c_int, 'int32_t': C.c_int32, 'int64_t': C.c_int64, 'unsigned': C.c_uint,
            'uint32_t': C.c_uint32, 'uint64_t': C.c_uint64, 'size_t': C.c_size_t,
            'float': C.c_float, 'double': C.c_double}
_POINTEES = set(_SCALARS) | {'void', 'char', 'uint8_t', 'uint16_t', 'int16_t'}       # may stand behind a `*`
_DECLARATOR = re.compile(r'(?:const\s+)?(\w+)\s*((?:\*\s*(?:const\s*)?)*)(\w+)?\s*(\[\s*\w*\s*\])?')

Header = collections.namedtuple('Header', 'constants structs signatures')


def parse_header(text):
    """Header(constants {TG_NAME: int}, structs {C name: Structure class}, signatures {tg_name: (restype,
    argtypes)}) of header text.  Raises TecoganHipError naming the declaration it does not fully understand."""
    constants, structs, signatures, handles, opaque = {}, {}, {}, set(), set()

    def refuse(decl, why):
        raise TecoganHipError(f'tecogan_hip.h: `{" ".join(decl.split())}`: {why}')

    def integer(expr, decl):
        """-1, 0x10, (16 * 64 * 64)"""
        expr = expr.strip()
        factors = expr[1:-1] if expr.startswith('(') and expr.endswith(')') else expr
        try:
            return math.prod(int(f, 0) for f in factors.split('*'))
        except ValueError:
            refuse(decl, f'`{expr}` is not an integer or a product of integers')

    def ctype(part, decl, where):
        """(ctypes type, declared name) of one parameter / field / return type."""
        m = _DECLARATOR.fullmatch(part.strip())
        if not m:
            refuse(decl, f'cannot parse `{part.strip()}`')
        base, stars, name, array = m.group(1), m.group(2).count('*'), m.group(3), m.group(4)
        if (where == 'return') != (name is None) or (array and where != 'param'):
            refuse(decl, f'cannot parse `{part.strip()}`')
        if not stars and not array:
            if base in _SCALARS:
                return _SCALARS[base], name
            if base in handles:
                return C.c_void_p, name
            if base == 'void' and where == 'return':
                return None, name
            refuse(decl, f'`{base}` is not a type this binding passes by value')
        if base not in _POINTEES and base not in handles and base not in structs and base not in opaque:
            refuse(decl, f'unknown type `{base}`')
        if stars == 1 and not array and base in structs and where != 'field':
            return C.POINTER(structs[base]), name
        return (C.c_char_p if base == 'char' and where == 'return' else C.c_void_p), name

    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    code, in_cplusplus = [], False
    for line in text.splitlines():
        s = line.strip()
        if s == '#ifdef __cplusplus':
            in_cplusplus = True
        elif in_cplusplus:
            if s not in ('extern "C" {', '}', '#endif', ''):
                refuse(s, 'unexpected inside #ifdef __cplusplus')
            in_cplusplus = s != '#endif'
        elif s.startswith('#'):
            m = re.fullmatch(r'#\s*define\s+(TG_\w+)\s+(.+)', s)
            if m:
                constants[m.group(1)] = integer(m.group(2), s)
            elif not re.fullmatch(r'#\s*(include\s*<\w+\.h>|ifndef\s+TECOGAN_HIP_H|define\s+TECOGAN_HIP_H|endif)', s):
                refuse(s, 'preprocessor line outside the parsing contract')
        else:
            code.append(line)

    # a declaration ends at a `;` outside braces
    code, decls, depth, start = '\n'.join(code), [], 0, 0
    for m in re.finditer(r'[;{}]', code):
        depth += (m.group() == '{') - (m.group() == '}')
        if m.group() == ';' and depth == 0:
            decls.append(code[start:m.start()].strip())
            start = m.end()
    if code[start:].strip():
        refuse(code[start:], 'declaration without its `;`')
    for decl in decls:
        m = re.fullmatch(r'typedef\s+void\s*\*\s*(\w+)', decl)
        if m:
            handles.add(m.group(1))
            continue
        m = re.fullmatch(r'typedef\s+struct\s+(\w+)\s+(\w+)', decl)
        if m:
            opaque.add(m.group(2))
            continue
        m = re.fullmatch(r'enum\s*\{([^{}]*)\}', decl)
        if m:
            for item in filter(None, (i.strip() for i in m.group(1).split(','))):
                k = re.fullmatch(r'(TG_\w+)\s*=\s*(.+)', item, flags=re.S)
                if not k:
                    refuse(decl, f'enumerator `{item}` needs the form TG_NAME = integer')
                constants[k.group(1)] = integer(k.group(2), decl)
            continue
        m = re.fullmatch(r'typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)', decl)
        if m:
            fields = []
            for stmt in filter(None, (s.strip() for s in m.group(1).split(';'))):
                first, *more = stmt.split(',')
                typ, name = ctype(first, decl, 'field')
                if more and (typ is C.c_void_p or not all(re.fullmatch(r'\s*\w+\s*', n) for n in more)):
                    refuse(decl, f'`{stmt}`: only plain scalars may share one declaration')
                fields += [(n.strip(), typ) for n in [name] + more]
            structs[m.group(2)] = type(m.group(2), (C.Structure,), {'_fields_': fields})
            continue
        m = re.fullmatch(r'([\w\s*]+?)\b(tg_\w+)\s*\((.*)\)', decl, flags=re.S)
        if not m or '(' in m.group(3) or '{' in decl or m.group(2) in signatures:
            refuse(decl, 'not a declaration this binding understands, or declared twice')
        params = m.group(3).strip()
        signatures[m.group(2)] = (ctype(m.group(1), decl, 'return')[0],
                                  [] if params == 'void' else [ctype(p, decl, 'param')[0] for p in params.split(',')])
    return Header(constants, structs, signatures)


try:
    with open(HEADER_PATH) as _f:
        _HEADER = parse_header(_f.read())
except OSError as e:
    raise TecoganHipError(f'{HEADER_PATH}: cannot read the C ABI header this binding is derived from ({e})')

globals().update(_HEADER.constants)                 # every enumerator and integer #define: _lib.TG_<NAME>
_K = _HEADER.constants
TG_OK, ABI_MAJOR = _K['TG_OK'], _K['TG_ABI_MAJOR']
ACT_NONE, ACT_RELU, ACT_LRELU02, ACT_TANH24 = (_K['TG_ACT_' + k] for k in ('NONE', 'RELU', 'LRELU02', 'TANH24'))
UP_NONE, UP_BICUBIC, UP_BILINEAR = (_K['TG_UP_' + k] for k in ('NONE', 'BICUBIC', 'BILINEAR'))
PREC_F32, PREC_F16 = _K['TG_PREC_F32'], _K['TG_PREC_F16']
YUV_MATRIX = {'bt601': _K['TG_YUV_BT601'], 'bt709': _K['TG_YUV_BT709']}
YUV_SITING = {'center': _K['TG_YUV_CENTER'], 'left': _K['TG_YUV_LEFT']}
# what the three tg_*yuv_planar* entry points take on top; YUV_MATRIX stays the 4:2:0 functions'
YUV_PLANAR_MATRIX = dict(YUV_MATRIX, bt2020=_K['TG_YUV_BT2020'])
YUV_CHROMA = {'420': _K['TG_YUV_420'], '422': _K['TG_YUV_422'], '444': _K['TG_YUV_444']}
PNG_FILTER = {'none': _K['TG_PNG_FILTER_NONE'], 'adaptive': _K['TG_PNG_FILTER_ADAPTIVE']}

STRUCTS = _HEADER.structs                           # C name -> Structure class
FrnetCfg, WinoLayer, ChainLayer = STRUCTS['tg_frnet_cfg'], STRUCTS['tg_wino_layer'], STRUCTS['tg_chain_layer']
PackedLayer, PackItem = STRUCTS['tg_packed_layer'], STRUCTS['tg_pack_item']
WresConvT, LayerWeights = STRUCTS['tg_wres_convt'], STRUCTS['tg_layer_weights']

SIGNATURES = _HEADER.signatures                     # name -> (restype, argtypes)

_lib = None


def lib():
    """Load (once) and return the ctypes handle; raises if the .so is absent."""
    global _lib
    if _lib is None:
        if not os.path.isfile(LIB_PATH):
            raise TecoganHipError(
                f'{LIB_PATH} not found: build it with '
                f'`bash {os.path.join(_HERE, "csrc", "build.sh")}` '
                '(hipcc --offload-arch=gfx950).  There is no CPU/ATen fallback.')
        # torch bundles its own HIP runtime; it must be the one already mapped
        # when our library (linked against libamdhip64) is opened, otherwise two
        # runtimes coexist and ours sees no device.
        import torch  # noqa: F401
        handle = C.CDLL(LIB_PATH)
        handle.tg_version.restype = C.c_int
        if handle.tg_version() // 100 != ABI_MAJOR:
            raise TecoganHipError(f'{LIB_PATH}: ABI {handle.tg_version()} but include/tecogan_hip.h declares '
                                  f'TG_ABI_MAJOR {ABI_MAJOR}: rebuild the library')
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)      # AttributeError if a symbol is missing
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


def check(rc, what):
    if rc != TG_OK:
        msg = lib().tg_last_error_string().decode('utf-8', 'replace')
        raise TecoganHipError(f'{what} failed (code {rc}): {msg}')
