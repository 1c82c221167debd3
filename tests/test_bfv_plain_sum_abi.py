"""The BFV plaintext-weighted sums exist through every layer (header, library, ctypes table, PhantomContext, documents); no compute,
no GPU."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STRIDES = ["size_t plain_term_stride", "size_t plain_batch_stride", "size_t ct_term_stride", "size_t ct_batch_stride",
           "size_t acc_batch_stride"]
SUM_TAIL = ["const uint64_t *ct", "const uint64_t *acc", "uint64_t *res", "size_t terms", "size_t batch"] + STRIDES + [
    "size_t chunk", "size_t slab", "void *stream"]
SUM_PARAMS = ["ct", "acc", "res", "terms", "batch", "strides", "chunk", "slab"]
# C entry -> (PhantomContext method, its parameters after self, the C argument list of include/phantom_amd.h written out)
ENTRIES = {
    "pha_bfv_lift_plain_batched": (
        "bfv_lift_plain_batched", ["size_Ql", "plain", "count", "out", "strides"],
        ["pha_context_t ctx", "size_t size_Ql", "const uint64_t *plain", "size_t count", "size_t plain_stride", "uint64_t *out",
         "size_t out_stride", "void *stream"]),
    "pha_bfv_multiply_plain_sum_batched": (
        "bfv_multiply_plain_sum_batched", ["size_Ql", "plain_ntt"] + SUM_PARAMS,
        ["pha_context_t ctx", "size_t size_Ql", "const uint64_t *plain_ntt"] + SUM_TAIL),
    "pha_bfv_plain_inner_product_batched": (
        "bfv_plain_inner_product_batched", ["size_Ql", "plain"] + SUM_PARAMS,
        ["pha_context_t ctx", "size_t size_Ql", "const uint64_t *plain"] + SUM_TAIL),
}


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_header_declares_the_entries_as_extensions():
    text = _read("include", "phantom_amd.h")
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, (_, _, want) in ENTRIES.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert m, f"{name} is not declared in include/phantom_amd.h"
        args = [" ".join(a.split()) for a in m.group(1).split(",")]
        assert args == want, f"{name}: {args}"
    assert [len(v[2]) for v in ENTRIES.values()] == [8, 16, 16]
    # next to pha_bfv_multiply_plain's family, documented
    lift = text.index("int pha_bfv_lift_plain_batched(")
    assert text.index("int pha_bfv_multiply_plain(") < lift < text.index("int pha_bfv_multiply_plain_sum_batched(") \
        < text.index("int pha_bfv_plain_inner_product_batched(")
    comment = text[text.rindex("/* Extension", 0, lift):text.index("int pha_bfv_plain_inner_product_batched(")]
    for needle in ("multiply_plain_normal", "pha_abs_plain_rns_poly", "pha_nwt_2d_radix8_forward_inplace", "load prologue",
                   "COEFFICIENT form", "[chunk][slab][2][L][N]", "chunk", "slab", "pha_bfv_multiply_plain", "pha_add_rns_poly",
                   "captured into a graph", "refused", "section 4.8d"):
        assert needle in comment, needle


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
            expect = ctypes.c_size_t if decl.startswith("size_t") else ctypes.c_void_p
            assert t is expect, f"{name}: {decl} bound as {t}"


def test_context_methods_exist_with_default_strides_chunk_and_slab():
    import phantom_fhe_amd as P
    for name, (method, params, _) in ENTRIES.items():
        fn = getattr(P.PhantomContext, method, None)
        assert callable(fn), f"PhantomContext.{method} is missing"
        sig = inspect.signature(fn)
        assert list(sig.parameters)[1:] == params, f"{method}{sig}"
        assert sig.parameters["strides"].default is None
        for key in ("chunk", "slab"):
            if key in params:
                assert sig.parameters[key].default == 0


def test_null_context_is_refused_with_a_message():
    from phantom_fhe_amd import lib as L
    lib = L.load()
    for name in ENTRIES:
        fn = getattr(lib, name)
        args = [None if t is ctypes.c_void_p else 1 for t in fn.argtypes]
        assert fn(*args) == -1, name
        assert b"null context" in lib.pha_last_error()
        with pytest.raises(ValueError):
            L.check(-1)


def test_the_other_layers_say_where_the_entries_are_and_are_not():
    names = list(ENTRIES)
    design = _read("DESIGN.md")
    assert "4.8d" in design
    section = design[design.index("4.8d"):]
    for needle in names + ["2·K·L + 2·L", "5·K·L", "[chunk][slab][2][L][N]", "EPI_INV_CANON_ADD", "PRO_LIFT"]:
        assert needle in section, f"DESIGN.md section 4.8d lacks {needle}"
    integration = _read("INTEGRATION.md")
    for name in names:
        assert name in integration, f"INTEGRATION.md does not list {name}"
    assert "pha_bfv_multiply_plain_sum_batched" in _read("README.md")
    assert os.path.exists(os.path.join(ROOT, "profiles", "bfv_plain_sum.md"))
    # host mirror and pyPhantom hold one buffer per object: the batched extensions are not there
    for path in (("phantom-fhe_amd", "host", "phantom.h"), ("phantom-fhe_amd", "python", "binding.cpp")):
        assert "bfv_multiply_plain_sum_batched" not in _read(*path)
