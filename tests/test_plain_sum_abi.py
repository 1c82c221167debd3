"""The plaintext-weighted sum and its rescale entry exist through every layer (header, library, ctypes table, PhantomContext);
no compute, no GPU."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# C entry -> (PhantomContext method, its parameters after self, the C argument list of include/phantom_amd.h written out)
STRIDES = ["size_t plain_term_stride", "size_t plain_batch_stride", "size_t ct_term_stride", "size_t ct_batch_stride",
           "size_t acc_batch_stride"]
ENTRIES = {
    "pha_multiply_plain_sum_batched": (
        "multiply_plain_sum_batched", ["plain", "ct", "acc", "res", "cms", "terms", "batch", "strides"],
        ["pha_context_t ctx", "const uint64_t *plain", "const uint64_t *ct", "const uint64_t *acc", "uint64_t *res",
         "size_t coeff_mod_size", "size_t terms", "size_t batch"] + STRIDES + ["void *stream"]),
    "pha_plain_inner_product_rescale_batched": (
        "plain_inner_product_rescale_batched", ["size_Ql", "plain", "ct", "acc", "terms", "batch", "scheme", "dst", "strides", "chunk"],
        ["pha_context_t ctx", "size_t size_Ql", "const uint64_t *plain", "const uint64_t *ct", "const uint64_t *acc", "size_t terms",
         "size_t batch"] + STRIDES + ["int scheme", "uint64_t *dst", "size_t chunk", "void *stream"]),
}


def _header():
    return open(os.path.join(ROOT, "include", "phantom_amd.h")).read()


def test_header_declares_the_entries_as_extensions():
    text = _header()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, (_, _, want) in ENTRIES.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert m, f"{name} is not declared in include/phantom_amd.h"
        args = [" ".join(a.split()) for a in m.group(1).split(",")]
        assert args == want, f"{name}: {args}"
    assert len(ENTRIES["pha_multiply_plain_sum_batched"][2]) == 14
    # after pha_inner_product_relin_batched, documented like their neighbours
    first = text.index("int pha_multiply_plain_sum_batched(")
    second = text.index("int pha_plain_inner_product_rescale_batched(")
    assert text.index("int pha_inner_product_relin_batched(") < first < second
    between = text[text.index("int pha_inner_product_relin_batched("):first]
    assert between.count("\nint ") == 0, "another entry sits between pha_inner_product_relin_batched and the new ones"
    comment = text[text.rindex("/*", 0, first):first]
    assert comment.startswith("/* Extension (no reference launcher")
    assert "multiply_rns_poly" in comment and "add_rns_poly" in comment and "multiply_and_add_rns_poly" in comment
    assert "rescale_to_next" in comment and "mod_switch_to_next" in comment
    assert "[L][N]" in comment and "[2][L][N]" in comment and "res [batch][2][L][N]" in comment
    comment2 = text[text.rindex("/*", 0, second):second]
    assert "dst [batch][2][Ql-1][N]" in comment2 and "bfv" in comment2 and "chunk" in comment2


def test_library_exports_and_binding_declares_them():
    import phantom_fhe_amd as P
    from phantom_fhe_amd import lib as L
    if not os.path.exists(P.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    so = ctypes.CDLL(P.LIB_PATH)
    for name, (_, _, want) in ENTRIES.items():
        assert hasattr(so, name), f"{name} is not exported by the built library"
        assert name in P.EXPORTED, f"{name} has no argtypes in phantom_fhe_amd/lib.py"
        fn = getattr(L.load(), name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(want), f"{name}: {fn.argtypes}"
        for t, decl in zip(fn.argtypes, want):
            expect = ctypes.c_size_t if decl.startswith("size_t") else ctypes.c_int if decl.startswith("int ") else ctypes.c_void_p
            assert t is expect, f"{name}: {decl} bound as {t}"
    assert L.load().pha_plain_inner_product_rescale_batched.argtypes[12] is ctypes.c_int       # scheme


def test_context_methods_exist_with_default_strides_and_chunk():
    import phantom_fhe_amd as P
    for name, (method, params, _) in ENTRIES.items():
        fn = getattr(P.PhantomContext, method, None)
        assert callable(fn), f"PhantomContext.{method} is missing"
        sig = inspect.signature(fn)
        assert list(sig.parameters)[1:] == params, f"{method}{sig}"
        assert sig.parameters["strides"].default is None
        if "chunk" in params:
            assert sig.parameters["chunk"].default == 0


def test_null_context_is_refused_with_a_message():
    """Without a HIP device there is no context to call the entries on, and the C entries refuse a null context with a message
    instead of computing anything somewhere else."""
    from phantom_fhe_amd import lib as L
    lib = L.load()
    for name in ENTRIES:
        fn = getattr(lib, name)
        args = [None if t is ctypes.c_void_p else 1 for t in fn.argtypes]
        assert fn(*args) == -1, name
        assert b"null context" in lib.pha_last_error()
        with pytest.raises(ValueError):
            L.check(-1)
