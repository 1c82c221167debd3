"""The noise entries exist through the layers that have them (header, library, ctypes table, PhantomContext, workloads); no
compute, no GPU."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# C entry -> (PhantomContext method, its parameters after self, the C argument list of include/phantom_amd.h written out)
ENTRIES = {
    "pha_poly_infty_norm_batched": (
        "poly_infty_norm_batched", ["size_Ql", "src", "bits", "norm", "scalar", "count", "stride"],
        ["pha_context_t ctx", "size_t size_Ql", "const uint64_t *src", "size_t count", "size_t src_stride", "uint64_t scalar",
         "uint64_t *norm", "uint32_t *bits", "void *stream"]),
    "pha_invariant_noise_budget_batched": (
        "invariant_noise_budget_batched",
        ["size_Ql", "ct", "sk_powers", "scheme", "budget", "norm", "cipher_size", "batch", "n_powers", "stride", "chunk"],
        ["pha_context_t ctx", "size_t size_Ql", "const uint64_t *ct", "size_t cipher_size", "size_t batch", "size_t ct_stride",
         "const uint64_t *sk_powers", "size_t n_powers", "int scheme", "int32_t *budget", "uint64_t *norm", "size_t chunk",
         "void *stream"]),
}


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_header_declares_and_documents_the_entries():
    text = _read("include", "phantom_amd.h")
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, (_, _, want) in ENTRIES.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert m, f"{name} is not declared in include/phantom_amd.h"
        args = [" ".join(a.split()) for a in m.group(1).split(",")]
        assert args == want, f"{name}: {args}"
    first = text.index("int pha_poly_infty_norm_batched(")
    assert first > text.index("int pha_decrypt_mod_t("), "the section follows decryption"
    assert first < text.index("int pha_encrypt_zero_symmetric_batched(")
    comment = text[text.rindex("/*", 0, first):first]
    for name in ENTRIES:
        assert name in comment, f"{name} is not described in the section's comment"
    flat = re.sub(r"\s*\n \*\s*", " ", comment)              # the comment's lines joined
    for word in ("src/secretkey.cu:752-840", "poly_infinity_norm_coeffmod", "max_j min(v_j, Q_l - v_j)", "little-endian", "0 for a zero norm",
                 "COEFFICIENT form", "scalar = t", "scalar = 1", "max(0, bitcount(Q_l) - bits - 1)", "may be NULL",
                 "Every `chunk` gives the same words", "only read", "an unknown scheme", "without a plain modulus", "overlapping an input",
                 "batch == 0", "No entry synchronises", "noise_budget ct", "noise_budget sk_powers", "poly_infty_norm src",
                 "no floating point, no atomics"):
        assert word in flat, word
    strict = text[text.index("pha_set_strict(on)"):text.index("int pha_check_canonical(")]
    for name in ENTRIES:
        assert name in strict, f"{name} is missing from the strict-mode list"


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
            expect = {"size_t": ctypes.c_size_t, "int": ctypes.c_int, "uint64_t": ctypes.c_uint64}.get(decl.split()[0], ctypes.c_void_p)
            if "*" in decl:
                expect = ctypes.c_void_p
            assert t is expect, f"{name}: {decl} bound as {t}"


def test_context_methods_and_workload_exist():
    import phantom_fhe_amd as P
    from phantom_fhe_amd import workloads as W
    for name, (method, params, _) in ENTRIES.items():
        fn = getattr(P.PhantomContext, method, None)
        assert callable(fn), f"PhantomContext.{method} is missing"
        sig = inspect.signature(fn)
        assert list(sig.parameters)[1:] == params, f"{method}{sig}"
        assert sig.parameters["norm"].default is None and sig.parameters["stride"].default is None
        if "chunk" in params:
            assert sig.parameters["chunk"].default == 0
    assert inspect.signature(P.PhantomContext.poly_infty_norm_batched).parameters["scalar"].default == 1
    assert list(inspect.signature(W.noise_budget_batch).parameters) == ["ctx", "cts", "level", "sk_powers", "scheme"]


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


def test_documents_place_the_feature():
    """invariant_noise_budget is at the C ABI and in phantom_fhe_amd, not in the host mirror or pyPhantom (no
    PhantomSecretKey there); DESIGN.md has section 4.15; the per-thread programs live in a header the host can compile."""
    text = _read("INTEGRATION.md")
    assert "invariant_noise_budget" in text and "pha_invariant_noise_budget_batched" in text
    host = _read("phantom-fhe_amd", "host", "phantom.h")
    assert "invariant_noise_budget" not in host and "class PhantomSecretKey" not in host
    assert "4.15" in _read("DESIGN.md")
    header = _read("phantom-fhe_amd", "csrc", "pha_noise.h")
    for fn in ("noise_garner", "noise_greater", "noise_magnitude", "noise_horner", "noise_bits", "noise_budget"):
        assert "PHA_HD" in header and fn in header, fn
