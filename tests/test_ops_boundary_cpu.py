"""The boundary rule of tecogan_pytorch_amd.ops, checked without a device and without the
library: one way in (ops._call), every operand checked before anything is allocated or launched.

ops._call is replaced by a recorder (tests/ops_cases.py), so a wrapper with a missing check fails a test here instead
of handing a host address to a kernel."""
import ast
import os
import re

import pytest

from tecogan_pytorch_amd import ops
from tecogan_pytorch_amd._lib import TecoganHipError
from tests import ops_cases as OC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(ops.__file__) as _f:
    OPS_SOURCE = _f.read()
OPS_TREE = ast.parse(OPS_SOURCE)
with open(os.path.join(ROOT, 'include', 'tecogan_hip.h')) as _f:
    HEADER = _f.read()


def stream_entry_points():
    """Names of the prototypes whose last parameter is a tg_stream_t: declarations end in `;`, and a prototype is the
    tg_ name in front of its one parenthesised parameter list."""
    text = re.sub(r'/\*.*?\*/', ' ', HEADER, flags=re.S)
    names = set()
    for decl in text.split(';'):
        m = re.search(r'\b(tg_\w+)\s*\(([^()]*)\)\s*$', decl.strip(), flags=re.S)
        if m and re.search(r'\btg_stream_t\s+\w+\s*$', m.group(2)):
            names.add(m.group(1))
    return names


@pytest.mark.parametrize('label,build,entry_names,host', OC.ROWS, ids=[r[0] for r in OC.ROWS])
def test_every_wrapper_refuses_host_tensors(monkeypatch, label, build, entry_names, host):
    """Every row built on the CPU raises TecoganHipError -- not AssertionError, not AttributeError -- and nothing
    reaches the library; fault_to_slot's counter is unpinned here, which is what it refuses."""
    seen = OC.recorder(monkeypatch, ops)
    fn, kwargs = build(ops, 'cpu')
    with pytest.raises(TecoganHipError):
        fn(**kwargs)
    assert seen == []


def test_rows_cover_every_entry_point_ops_calls():
    """The string literals passed as the first argument of _call( in ops.py are the union of the rows' entry names: a
    new wrapper without a row fails here.  Where the first argument is a choice between two literals both count; where
    it is a plain variable (the table-driven YUV bodies, png_encode, downsample_bi) the literal stands elsewhere in the
    module, so every string constant of ops.py that names a stream-taking prototype counts as well."""
    firsts = [n.args[0] for n in ast.walk(OPS_TREE)
              if isinstance(n, ast.Call) and isinstance(n.func, ast.Name) and n.func.id == '_call']
    assert len(firsts) > 100 and all(isinstance(a, (ast.Constant, ast.IfExp, ast.Name)) for a in firsts)
    literal = {c.value for a in firsts for c in ast.walk(a) if isinstance(c, ast.Constant) and isinstance(c.value, str)}
    streamed = stream_entry_points()
    literal |= {n.value for n in ast.walk(OPS_TREE) if isinstance(n, ast.Constant) and n.value in streamed}
    covered = set().union(*(r[2] for r in OC.ROWS))
    assert literal <= streamed, sorted(literal - streamed)
    assert literal == covered, (sorted(literal - covered), sorted(covered - literal))


def test_every_launch_goes_through_call_and_no_assert_is_left():
    streamed = stream_entry_points()
    # the scan found every prototype there is: tg_stream_t is always the last parameter, one per prototype
    assert len(streamed) == len(re.findall(r'\btg_stream_t\s+\w+\s*\)\s*;', HEADER)) > 100
    assert not re.search(r'\btg_stream_t\s+\w+\s*,', HEADER)
    assert 'tg_conv3x3_fwd' in streamed and 'tg_conv3x3_pick_ocb' not in streamed
    direct = sorted({n.attr for n in ast.walk(OPS_TREE) if isinstance(n, ast.Attribute) and n.attr in streamed})
    assert direct == [], f'ops.py reaches {direct} without _call'
    asserts = [n.lineno for n in ast.walk(OPS_TREE) if isinstance(n, ast.Assert)]
    assert asserts == [], f'ops.py: assert statements at lines {asserts} (they vanish under python -O)'
    assert not re.search(r'^\s*assert\b', OPS_SOURCE, flags=re.M)
