"""The fp16-input CSR entries at the C boundary, without a GPU: declared, exported,
bound, and their argument checks (made before any device work) in the order of the
fp32 entries'."""
from __future__ import annotations

import os
import re
import subprocess

from conftest import ROOT

NAMES = ("spmm_csrmm_ex_f16", "spmm_gespmm_csrmm_f16")


def test_declared_exported_and_bound():
    from spmm_hip import _lib
    src = open(os.path.join(ROOT, "include", "spmm_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", src), name + " is not declared"
        assert name in exported, name + " is not exported"
        assert name in _lib.EXPORTED
        f32 = name.replace("_f16", "_f32")
        assert _lib._PROTOS[name] == _lib._PROTOS[f32], "the fp32 entry's argument list"


def test_host_side_checks_match_the_f32_entries():
    from spmm_hip import _lib
    L = _lib.lib()
    for ex in (L.spmm_csrmm_ex_f16, L.spmm_csrmm_ex_f32):
        # a null handle comes first, whatever else is wrong
        assert ex(None, 1, 1, 1, 0, 1.0, None, None, None, 0, None, 1, 0, 0.0, None, 1, 0) == 1
        assert ex(None, -1, 1, 1, 0, 1.0, None, None, None, 7, None, 1, 0, 0.0, None, 1, 0) == 1
    for ge in (L.spmm_gespmm_csrmm_f16, L.spmm_gespmm_csrmm_f32):
        assert ge(-1, 4, None, None, None, None, None, None) == 3
        assert ge(4, -1, None, None, None, None, None, None) == 3
        assert ge(0, 4, None, None, None, None, None, None) == 0  # quick return
        assert ge(4, 0, None, None, None, None, None, None) == 0
        assert ge(4, 4, None, None, None, None, None, None) == 3


def test_python_wrappers_exist_and_take_halves_only():
    import inspect

    from spmm_hip import ops
    assert "csrmm_f16" in ops.__all__ and "gespmm_csrmm_f16" in ops.__all__
    a, b = inspect.signature(ops.csrmm_f16), inspect.signature(ops.csrmm)
    assert list(a.parameters) == list(b.parameters)
    assert [p.default for p in a.parameters.values()] == [p.default for p in b.parameters.values()]
    assert list(inspect.signature(ops.gespmm_csrmm_f16).parameters) == \
        list(inspect.signature(ops.gespmm_csrmm).parameters)
