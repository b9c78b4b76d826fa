"""The boundary rule of tecogan_pytorch_amd.ops on the device: for every row of
tests/ops_cases.py the valid call reaches the library, and with any one tensor operand replaced by a CPU copy, by
another dtype or by a non-contiguous tensor of the same shape it is refused before anything reaches it.

ops._call stays replaced by the recorder of tests/ops_cases.py: no kernel is launched, the rows allocate a few
kilobytes each."""
import pytest
import torch

from tecogan_pytorch_amd import ops
from tecogan_pytorch_amd._lib import TecoganHipError
from tests import ops_cases as OC

pytestmark = pytest.mark.gpu

OTHER_DTYPE = {torch.float32: torch.float64, torch.float16: torch.float64, torch.float64: torch.float32,
               torch.uint8: torch.int32, torch.uint16: torch.int32, torch.int64: torch.int32, torch.int32: torch.int64}


def bad_versions(t, host):
    """(what, tensor) replacements of operand t, each of t's shape: a CPU copy (not for an operand that is host memory
    by design, which stays pinned in the other two), another dtype, and a tensor none of whose dimensions is dense --
    which exists only for a shape with more than one element."""
    pin = (lambda x: x.pin_memory()) if host else (lambda x: x)
    if not host:
        yield 'cpu', t.cpu()
    yield 'dtype', pin(torch.empty(t.shape, dtype=OTHER_DTYPE[t.dtype], device=t.device))
    if t.numel() > 1:
        wide = pin(torch.empty(*t.shape, 2, dtype=t.dtype, device=t.device))[..., 0]
        assert wide.shape == t.shape and not wide.is_contiguous()
        yield 'strided', wide


@pytest.mark.parametrize('label,build,entry_names,host', OC.ROWS, ids=[r[0] for r in OC.ROWS])
def test_valid_call_passes_and_every_bad_operand_is_refused(monkeypatch, label, build, entry_names, host):
    seen = OC.recorder(monkeypatch, ops)
    fn, kwargs = build(ops, 'cuda')
    try:
        fn(**kwargs)
    except OC.Stop:
        pass
    assert seen and set(seen) <= entry_names, f'{label}: reached {seen}, the row allows {sorted(entry_names)}'
    operands = list(OC.tensor_paths(kwargs))
    assert operands, label
    for path, t in operands:
        for what, bad in bad_versions(t, path[0] in host):
            del seen[:]
            with pytest.raises(TecoganHipError):
                fn(**OC.replaced(kwargs, path, bad))
                pytest.fail(f'{label}: {what} tensor for {path} was accepted (reached {seen})')
            assert seen == [], f'{label}: {what} tensor for {path}: {seen} was reached before the refusal'
