"""The batched hoisted rotations exist through every layer (header, both libraries, ctypes table, PhantomContext, workloads); no
compute, no GPU."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# C entry -> (PhantomContext method, its parameters after self, the C arguments of include/phantom_amd.h written out)
ENTRIES = {
    "pha_hoisting_batched": (
        "hoisting_batched", ["size_Ql", "ct", "galois_elts", "galois_keys", "scheme", "out", "chunk"],
        ["pha_context_t ctx", "size_t size_Ql", "const uint64_t *ct", "size_t batch", "const uint32_t *galois_elts", "size_t n_elts",
         "const uint64_t *const *const *glk", "int scheme", "uint64_t *out", "size_t chunk", "void *stream"]),
    "pha_hoisting_weighted_batched": (
        "hoisting_weighted_batched", ["size_Ql", "ct", "galois_elts", "galois_keys", "weights", "scheme", "out", "chunk"],
        ["pha_context_t ctx", "size_t size_Ql", "const uint64_t *ct", "size_t batch", "const uint32_t *galois_elts", "size_t n_elts",
         "const uint64_t *const *const *glk", "const uint64_t *const *weights", "int scheme", "uint64_t *out", "size_t chunk",
         "void *stream"]),
}


def test_header_declares_the_entries_where_the_issue_puts_them():
    text = open(os.path.join(ROOT, "include", "phantom_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, (_, _, want) in ENTRIES.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert m, f"{name} is not declared in include/phantom_amd.h"
        assert [" ".join(a.split()) for a in m.group(1).split(",")] == want, name
    at = {n: code.index("int " + n + "(") for n in list(ENTRIES) + ["pha_hoisting_weighted_bsgs_blocks", "pha_generate_one_kswitch_key"]}
    # directly after pha_hoisting_weighted_bsgs_blocks and before pha_generate_one_kswitch_key, nothing else in between
    assert at["pha_hoisting_weighted_bsgs_blocks"] < at["pha_hoisting_batched"] < at["pha_hoisting_weighted_batched"] \
        < at["pha_generate_one_kswitch_key"]
    between = code[at["pha_hoisting_weighted_bsgs_blocks"]:at["pha_generate_one_kswitch_key"]]
    assert re.findall(r"\bint\s+(pha_\w+)\s*\(", between) == ["pha_hoisting_weighted_bsgs_blocks"] + list(ENTRIES)
    strict = text[text.index(" * pha_set_strict(on)"):text.index("int pha_check_canonical(")]
    for name in ENTRIES:
        assert name in strict, f"{name} is not listed with the strict-mode entries"


def test_both_libraries_export_and_the_binding_declares_them():
    import phantom_fhe_amd as P
    from phantom_fhe_amd import lib as L
    if not os.path.exists(P.LIB_PATH) or not os.path.exists(P.EXP_LIB_PATH):
        import __graft_entry__ as g
        g.build()
    for path in (P.LIB_PATH, P.EXP_LIB_PATH):
        so = ctypes.CDLL(path)
        for name in ENTRIES:
            assert hasattr(so, name), f"{name} is not exported by {os.path.basename(path)}"
    for name, (_, _, want) in ENTRIES.items():
        assert name in P.EXPORTED, f"{name} has no argtypes in phantom_fhe_amd/lib.py"
        fn = getattr(L.load(), name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(want), f"{name}: {fn.argtypes}"
        for t, arg in zip(fn.argtypes, want):
            if arg.startswith("size_t "):
                assert t is ctypes.c_size_t, f"{name}: {arg} bound as {t}"
            elif arg.startswith("int "):
                assert t is ctypes.c_int, f"{name}: {arg} bound as {t}"
            elif arg.startswith("const uint32_t *"):
                assert t is ctypes.POINTER(ctypes.c_uint32), f"{name}: {arg} bound as {t}"
            elif "*const *" in arg:
                assert t is ctypes.POINTER(ctypes.c_void_p), f"{name}: {arg} bound as {t}"
            else:
                assert t is ctypes.c_void_p, f"{name}: {arg} bound as {t}"


def test_context_methods_and_the_workload_exist_with_their_defaults():
    import phantom_fhe_amd as P
    from phantom_fhe_amd import workloads as W
    for name, (method, params, _) in ENTRIES.items():
        fn = getattr(P.PhantomContext, method, None)
        assert callable(fn), f"PhantomContext.{method} is missing"
        sig = inspect.signature(fn)
        assert list(sig.parameters)[1:] == params, f"{method}{sig}"
        for p in params:
            default = sig.parameters[p].default
            if p == "out":
                assert default is None
            elif p == "chunk":
                assert default == 0
            else:
                assert default is inspect.Parameter.empty, f"{method}: {p}"
    fn = getattr(W, "diag_matvec_batch", None)
    assert callable(fn), "workloads.diag_matvec_batch is missing"
    sig = inspect.signature(fn)
    assert list(sig.parameters) == ["ctx", "size_Ql", "cts", "galois_elts", "galois_keys", "diagonals", "scheme", "chunk"]
    assert sig.parameters["chunk"].default == 0
    assert all(sig.parameters[p].default is inspect.Parameter.empty for p in list(sig.parameters)[:-1])


def test_null_context_is_refused_with_a_message():
    from phantom_fhe_amd import lib as L
    lib = L.load()
    for name in ENTRIES:
        fn = getattr(lib, name)
        args = [2 if t in (ctypes.c_size_t, ctypes.c_int) else None for t in fn.argtypes]
        assert fn(*args) == -1, name
        assert b"null context" in lib.pha_last_error()
        with pytest.raises(ValueError):
            L.check(-1)
