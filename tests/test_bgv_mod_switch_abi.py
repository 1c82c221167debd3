"""The BGV key switch fused with mod_switch_to_next exists through every layer (header, both libraries, ctypes table,
PhantomContext); no compute, no GPU."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# C entry -> (PhantomContext method, its parameters after self, the C arguments of include/phantom_amd.h written out)
ENTRIES = {
    "pha_keyswitch_mod_switch": (
        "keyswitch_mod_switch", ["size_Ql", "ct", "c2", "rlk_ptrs", "dst"],
        ["pha_context_t ctx", "size_t size_Ql", "const uint64_t *ct", "const uint64_t *c2", "const uint64_t *const *rlk", "uint64_t *dst",
         "void *stream"]),
    "pha_keyswitch_mod_switch_batched": (
        "keyswitch_mod_switch_batched", ["size_Ql", "ct", "c2", "batch", "rlk_ptrs", "dst"],
        ["pha_context_t ctx", "size_t size_Ql", "const uint64_t *ct", "const uint64_t *c2", "size_t batch", "const uint64_t *const *rlk",
         "uint64_t *dst", "void *stream"]),
    "pha_inner_product_relin_mod_switch_batched": (
        "inner_product_relin_mod_switch_batched", ["size_Ql", "op1", "op2", "terms", "batch", "rlk_ptrs", "dst", "strides", "chunk"],
        ["pha_context_t ctx", "size_t size_Ql", "const uint64_t *op1", "const uint64_t *op2", "size_t terms", "size_t batch",
         "size_t op1_term_stride", "size_t op1_batch_stride", "size_t op2_term_stride", "size_t op2_batch_stride",
         "const uint64_t *const *rlk", "uint64_t *dst", "size_t chunk", "void *stream"]),
}


def test_header_declares_the_entries_where_the_issue_puts_them():
    text = open(os.path.join(ROOT, "include", "phantom_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, (_, _, want) in ENTRIES.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert m, f"{name} is not declared in include/phantom_amd.h"
        assert [" ".join(a.split()) for a in m.group(1).split(",")] == want, name
    at = {n: code.index("int " + n + "(") for n in list(ENTRIES) + ["pha_keyswitch_rescale_batched", "pha_tensor_prod_2x2_batched",
                                                                   "pha_inner_product_relin_batched", "pha_plain_inner_product_rescale_batched", "pha_hoisting"]}
    assert at["pha_keyswitch_rescale_batched"] < at["pha_keyswitch_mod_switch"] < at["pha_keyswitch_mod_switch_batched"] \
        < at["pha_tensor_prod_2x2_batched"]
    # after pha_inner_product_relin_batched, and behind the plaintext sums whose place right after it is pinned already
    assert at["pha_inner_product_relin_batched"] < at["pha_plain_inner_product_rescale_batched"] \
        < at["pha_inner_product_relin_mod_switch_batched"] < at["pha_hoisting"]
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
            assert t is (ctypes.c_size_t if arg.startswith("size_t ") else ctypes.c_void_p), f"{name}: {arg} bound as {t}"


def test_context_methods_exist_with_their_defaults():
    import phantom_fhe_amd as P
    for name, (method, params, _) in ENTRIES.items():
        fn = getattr(P.PhantomContext, method, None)
        assert callable(fn), f"PhantomContext.{method} is missing"
        sig = inspect.signature(fn)
        assert list(sig.parameters)[1:] == params, f"{method}{sig}"
        for p in params:
            default = sig.parameters[p].default
            if p == "strides":
                assert default is None
            elif p == "chunk":
                assert default == 0
            else:
                assert default is inspect.Parameter.empty, f"{method}: {p}"


def test_null_context_is_refused_with_a_message():
    from phantom_fhe_amd import lib as L
    lib = L.load()
    for name in ENTRIES:
        fn = getattr(lib, name)
        args = [None if t is ctypes.c_void_p else 2 for t in fn.argtypes]
        assert fn(*args) == -1, name
        assert b"null context" in lib.pha_last_error()
        with pytest.raises(ValueError):
            L.check(-1)
