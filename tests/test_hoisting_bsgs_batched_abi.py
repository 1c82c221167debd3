"""The batched baby-step / giant-step hoisted rotations exist through every layer (header, both libraries, ctypes table,
PhantomContext, workloads); no compute, no GPU."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAME = "pha_hoisting_weighted_bsgs_batched"
METHOD = "hoisting_weighted_bsgs_batched"
PARAMS = ["size_Ql", "ct", "baby_elts", "baby_keys", "giant_elts", "giant_keys", "weights", "scheme", "out", "chunk"]
# the C arguments of include/phantom_amd.h written out
C_ARGS = ["pha_context_t ctx", "size_t size_Ql", "const uint64_t *ct", "size_t batch", "const uint32_t *baby_elts", "size_t n_baby",
          "const uint64_t *const *const *baby_glk", "const uint32_t *giant_elts", "size_t n_giant",
          "const uint64_t *const *const *giant_glk", "const uint64_t *const *weights", "int scheme", "uint64_t *out", "size_t chunk",
          "void *stream"]


def test_header_declares_the_entry_where_the_issue_puts_it():
    text = open(os.path.join(ROOT, "include", "phantom_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^)]*)\)\s*;", code)
    assert m, f"{NAME} is not declared in include/phantom_amd.h"
    assert [" ".join(a.split()) for a in m.group(1).split(",")] == C_ARGS
    # directly after pha_hoisting_weighted_bsgs and before pha_hoisting_weighted_bsgs_blocks, nothing else in between
    at = {n: code.index("int " + n + "(") for n in ("pha_hoisting_weighted_bsgs", NAME, "pha_hoisting_weighted_bsgs_blocks")}
    assert at["pha_hoisting_weighted_bsgs"] < at[NAME] < at["pha_hoisting_weighted_bsgs_blocks"]
    between = code[at["pha_hoisting_weighted_bsgs"]:at["pha_hoisting_weighted_bsgs_blocks"]]
    assert re.findall(r"\bint\s+(pha_\w+)\s*\(", between) == ["pha_hoisting_weighted_bsgs", NAME]
    strict = text[text.index(" * pha_set_strict(on)"):text.index("int pha_check_canonical(")]
    assert NAME in strict, f"{NAME} is not listed with the strict-mode entries"


def test_both_libraries_export_and_the_binding_declares_it():
    import phantom_fhe_amd as P
    from phantom_fhe_amd import lib as L
    if not os.path.exists(P.LIB_PATH) or not os.path.exists(P.EXP_LIB_PATH):
        import __graft_entry__ as g
        g.build()
    for path in (P.LIB_PATH, P.EXP_LIB_PATH):
        assert hasattr(ctypes.CDLL(path), NAME), f"{NAME} is not exported by {os.path.basename(path)}"
    assert NAME in P.EXPORTED, f"{NAME} has no argtypes in phantom_fhe_amd/lib.py"
    fn = getattr(L.load(), NAME)
    assert fn.argtypes is not None and len(fn.argtypes) == len(C_ARGS), f"{NAME}: {fn.argtypes}"
    for t, arg in zip(fn.argtypes, C_ARGS):
        if arg.startswith("size_t "):
            assert t is ctypes.c_size_t, f"{arg} bound as {t}"
        elif arg.startswith("int "):
            assert t is ctypes.c_int, f"{arg} bound as {t}"
        elif arg.startswith("const uint32_t *"):
            assert t is ctypes.POINTER(ctypes.c_uint32), f"{arg} bound as {t}"
        elif "*const *" in arg:
            assert t is ctypes.POINTER(ctypes.c_void_p), f"{arg} bound as {t}"
        else:
            assert t is ctypes.c_void_p, f"{arg} bound as {t}"


def test_context_method_and_the_workload_exist_with_their_defaults():
    import phantom_fhe_amd as P
    from phantom_fhe_amd import workloads as W
    fn = getattr(P.PhantomContext, METHOD, None)
    assert callable(fn), f"PhantomContext.{METHOD} is missing"
    sig = inspect.signature(fn)
    assert list(sig.parameters)[1:] == PARAMS, f"{METHOD}{sig}"
    for p in PARAMS:
        default = sig.parameters[p].default
        if p == "out":
            assert default is None
        elif p == "chunk":
            assert default == 0
        else:
            assert default is inspect.Parameter.empty, f"{METHOD}: {p}"
    fn = getattr(W, "diag_matvec_bsgs_batch", None)
    assert callable(fn), "workloads.diag_matvec_bsgs_batch is missing"
    sig = inspect.signature(fn)
    assert list(sig.parameters) == ["ctx", "size_Ql", "cts", "baby_elts", "baby_keys", "giant_elts", "giant_keys", "diagonals", "scheme",
                                    "chunk"]
    assert sig.parameters["chunk"].default == 0
    assert all(sig.parameters[p].default is inspect.Parameter.empty for p in list(sig.parameters)[:-1])


def test_null_context_is_refused_with_a_message():
    from phantom_fhe_amd import lib as L
    lib = L.load()
    fn = getattr(lib, NAME)
    args = [2 if t in (ctypes.c_size_t, ctypes.c_int) else None for t in fn.argtypes]
    assert fn(*args) == -1
    assert b"null context" in lib.pha_last_error()
    with pytest.raises(ValueError):
        L.check(-1)
