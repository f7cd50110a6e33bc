"""The single-kernel entry points of the DAC's small kernels and the softmaxes (tests/test_gpu_dac_kernels.py): the header declares each one,
`_lib.SIGNATURES` declares the same names with the same number and kind of arguments, and the ABI version did not move.  No GPU."""
from __future__ import annotations

import ctypes as C
import os
import re

from tests.golden_defs import ROOT

from echo_tts_amd import _lib as L

ENTRIES = {
    "echo_op_dac_dwconv_ln": 14,
    "echo_op_dac_conv_out_tanh": 11,
    "echo_op_dac_snake": 8,
    "echo_op_dac_rope": 9,
    "echo_op_dac_conv_in_snake": 11,
    "echo_op_dac_vq_argmax": 12,
    "echo_op_softmax": 13,
}


def _header():
    with open(os.path.join(ROOT, "include", "echo_hip.h"), encoding="utf-8") as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def _kind(decl: str):
    """C parameter declaration -> the ctypes type `_lib.py` must use for it."""
    decl = decl.strip()
    if "*" in decl:
        return C.c_void_p
    ctype = decl.rsplit(None, 1)[0]
    return {"int": C.c_int, "int64_t": C.c_int64, "float": C.c_float}[ctype]


def test_header_and_ctypes_declare_the_same_entries():
    text = _header()
    for name, nargs in ENTRIES.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared in include/echo_hip.h"
        params = [p for p in m.group(1).split(",") if p.strip()]
        assert len(params) == nargs, (name, len(params))
        assert name in L.SIGNATURES, f"{name} is missing from _lib.SIGNATURES"
        res, args = L.SIGNATURES[name]
        assert res is C.c_int
        assert list(args) == [_kind(p) for p in params], name
        assert params[-1].split()[-1] == "stream"


def test_entries_are_defined_next_to_the_other_single_kernel_entries():
    with open(os.path.join(ROOT, "echo-tts_amd", "csrc", "engine.hip"), encoding="utf-8") as f:
        src = f.read()
    start = src.index("// ---- single-kernel entry points")
    for name in ENTRIES:
        assert re.search(r"^int " + name + r"\(", src[start:], flags=re.M), f"{name} is not defined in csrc/engine.hip"


def test_abi_version_is_still_8():
    with open(os.path.join(ROOT, "include", "echo_hip.h"), encoding="utf-8") as f:
        assert re.search(r"#define\s+ECHO_ABI_VERSION\s+8\b", f.read())
    assert L.ABI_VERSION == 8
