"""The summed tensor product and the two inner-product entries exist through every layer (header, library, ctypes table,
PhantomContext); no compute, no GPU."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# C entry -> (PhantomContext method, its parameters after self, number of C arguments: the prototypes of include/phantom_amd.h
# written out -- context, [size_Ql,] operands, [results,] [coeff_mod_size,] terms, batch, four strides, [key, [scheme,] dst, chunk,] stream)
ENTRIES = {
    "pha_tensor_prod_2x2_sum_batched": ("tensor_prod_2x2_sum_batched",
                                        ["op1", "op2", "res01", "res2", "cms", "terms", "batch", "strides"], 13),
    "pha_inner_product_relin_rescale_batched": ("inner_product_relin_rescale_batched",
                                                ["size_Ql", "op1", "op2", "terms", "batch", "rlk_ptrs", "dst", "strides", "chunk"], 14),
    "pha_inner_product_relin_batched": ("inner_product_relin_batched",
                                        ["size_Ql", "op1", "op2", "terms", "batch", "rlk_ptrs", "scheme", "dst", "strides", "chunk"], 15),
}
STRIDES = ["size_t op1_term_stride", "size_t op1_batch_stride", "size_t op2_term_stride", "size_t op2_batch_stride"]


def _header():
    return open(os.path.join(ROOT, "include", "phantom_amd.h")).read()


def test_header_declares_the_entries_as_extensions():
    text = _header()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, (_, _, argc) in ENTRIES.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert m, f"{name} is not declared in include/phantom_amd.h"
        args = [" ".join(a.split()) for a in m.group(1).split(",")]
        assert len(args) == argc, f"{name}: {len(args)} arguments {args}"
        assert args[0] == "pha_context_t ctx" and args[-1] == "void *stream"
        assert "size_t terms" in args and "size_t batch" in args
        at = args.index(STRIDES[0])
        assert args[at:at + 4] == STRIDES, f"{name}: {args}"
        if name != "pha_tensor_prod_2x2_sum_batched":
            assert args[1] == "size_t size_Ql" and args[-2] == "size_t chunk", f"{name}: {args}"
    # after pha_tensor_prod_2x2_batched, documented like their neighbours
    first = text.index("int pha_tensor_prod_2x2_sum_batched(")
    assert text.index("int pha_tensor_prod_2x2_batched(") < first < text.index("int pha_inner_product_relin_rescale_batched(") \
        < text.index("int pha_inner_product_relin_batched(")
    comment = text[text.rindex("/*", 0, first):first]
    assert comment.startswith("/* Extension (no reference launcher")
    assert "[2][L][N]" in comment and "res01 [batch][2][L][N], res2 [batch][L][N]" in comment
    assert "dst [batch][2][Ql-1][N]" in text and "dst [batch][2][Ql][N]" in text


def test_library_exports_and_binding_declares_them():
    import phantom_fhe_amd as P
    from phantom_fhe_amd import lib as L
    if not os.path.exists(P.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    so = ctypes.CDLL(P.LIB_PATH)
    for name, (_, _, argc) in ENTRIES.items():
        assert hasattr(so, name), f"{name} is not exported by the built library"
        assert name in P.EXPORTED, f"{name} has no argtypes in phantom_fhe_amd/lib.py"
        fn = getattr(L.load(), name)
        assert fn.argtypes is not None and len(fn.argtypes) == argc, f"{name}: {fn.argtypes}"
        assert fn.argtypes[-1] is ctypes.c_void_p
    assert L.load().pha_inner_product_relin_batched.argtypes[11] is ctypes.c_int       # scheme


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
    """Without a HIP device there is no context to call the entries on (PhantomContext raises), and the C entries refuse a null
    context with a message instead of computing anything somewhere else."""
    import torch
    import phantom_fhe_amd as P
    from phantom_fhe_amd import lib as L
    lib = L.load()
    for name, (_, _, argc) in ENTRIES.items():
        fn = getattr(lib, name)
        args = [None if t is ctypes.c_void_p else 1 for t in fn.argtypes]
        assert fn(*args) == -1, name
        assert b"null context" in lib.pha_last_error()
        with pytest.raises(ValueError):
            L.check(-1)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            P.PhantomContext(12, [0xffffee001, 0xffffc4001, 0x1ffffe0001], 1)
