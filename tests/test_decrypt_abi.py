"""The decryption entries exist through the layers that have them (header, library, ctypes table, PhantomContext, workloads);
no compute, no GPU."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BATCH_HEAD = ["pha_context_t ctx", "size_t size_Ql", "const uint64_t *ct", "size_t cipher_size", "size_t batch", "size_t ct_stride",
              "const uint64_t *sk_powers", "size_t n_powers"]
# C entry -> (PhantomContext method, its parameters after self, the C argument list of include/phantom_amd.h written out)
ENTRIES = {
    "pha_secret_key_powers": (
        "secret_key_powers", ["sk_ntt", "max_power", "out"],
        ["pha_context_t ctx", "const uint64_t *sk_ntt", "size_t max_power", "uint64_t *out", "void *stream"]),
    "pha_decrypt_phase_batched": (
        "decrypt_phase_batched", ["size_Ql", "ct", "sk_powers", "dst", "cipher_size", "batch", "n_powers", "strides"],
        BATCH_HEAD + ["uint64_t *dst", "size_t dst_stride", "void *stream"]),
    "pha_bgv_decrypt_batched": (
        "bgv_decrypt_batched", ["size_Ql", "ct", "sk_powers", "dst", "correction_factors", "cipher_size", "batch", "n_powers", "strides", "chunk"],
        BATCH_HEAD + ["const uint64_t *correction_factors", "uint64_t *dst", "size_t dst_stride", "size_t chunk", "void *stream"]),
    "pha_bfv_decrypt_batched": (
        "bfv_decrypt_batched", ["size_Ql", "ct", "sk_powers", "dst", "cipher_size", "batch", "n_powers", "strides", "chunk"],
        BATCH_HEAD + ["uint64_t *dst", "size_t dst_stride", "size_t chunk", "void *stream"]),
    "pha_hps_decrypt_scale_and_round": (
        "hps_decrypt_scale_and_round", ["size_Ql", "dst", "src"],
        ["pha_context_t ctx", "size_t size_Ql", "uint64_t *dst", "const uint64_t *src", "void *stream"]),
    "pha_decrypt_mod_t": (
        "decrypt_mod_t", ["size_Ql", "dst", "src"],
        ["pha_context_t ctx", "size_t size_Ql", "uint64_t *dst", "const uint64_t *src", "void *stream"]),
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
    first = text.index("int pha_secret_key_powers(")
    comment = text[text.rindex("/*", 0, first):first]
    for name in ENTRIES:
        assert name in comment, f"{name} is not described in the section's comment"
    for word in ("src/secretkey.cu:533-691", "compute_secret_key_array", "[max_power][size_QP][N]", "dst may be ct", "HOST array",
                 "invalid correction factor", "status -2", "COEFFICIENT form", "hps_overq_leveled", "Every `chunk` gives", "batch == 0",
                 "can be captured into a graph", "<entry> ct", "<entry> sk_powers", "writes 0", "L * 2^-14"):
        assert word in comment, word
    strict = text[text.index("pha_set_strict(on)"):text.index("int pha_check_canonical(")]
    for name in ("pha_decrypt_phase_batched", "pha_bgv_decrypt_batched", "pha_bfv_decrypt_batched"):
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
            if decl == "const uint64_t *correction_factors":      # a HOST array
                assert t is L.u64p, f"{name}: {decl} bound as {t}"
                continue
            expect = ctypes.c_size_t if decl.startswith("size_t") else ctypes.c_void_p
            assert t is expect, f"{name}: {decl} bound as {t}"


def test_context_methods_and_workload_exist():
    import phantom_fhe_amd as P
    from phantom_fhe_amd import workloads as W
    for name, (method, params, _) in ENTRIES.items():
        fn = getattr(P.PhantomContext, method, None)
        assert callable(fn), f"PhantomContext.{method} is missing"
        sig = inspect.signature(fn)
        assert list(sig.parameters)[1:] == params, f"{method}{sig}"
        if "strides" in params:
            assert sig.parameters["strides"].default is None
        if "chunk" in params:
            assert sig.parameters["chunk"].default == 0
    assert list(inspect.signature(W.decrypt_decode_batch).parameters) == ["ctx", "encoder", "cts", "level", "scale", "sk_powers"]


def test_null_context_is_refused_with_a_message():
    from phantom_fhe_amd import lib as L
    lib = L.load()
    for name in ENTRIES:
        fn = getattr(lib, name)
        args = [None if t in (ctypes.c_void_p, L.u64p) else 1 for t in fn.argtypes]
        assert fn(*args) == -1, name
        assert b"null context" in lib.pha_last_error()
        with pytest.raises(ValueError):
            L.check(-1)


def test_host_mirror_and_pyphantom_do_not_decrypt_yet():
    """decryption stops at the C ABI and phantom_fhe_amd; PhantomSecretKey, the two DRNSTool launchers and
    pyPhantom.secret_key stay absent, with everything else the issue leaves out."""
    host = _read("phantom-fhe_amd", "host", "phantom.h")
    assert "class PhantomSecretKey" not in host
    tool = host[host.index("class DRNSTool {"):host.index("class ContextData {")]
    for name in ("hps_decrypt_scale_and_round", "decrypt_mod_t", "behz_decrypt_scale_and_round"):
        assert name not in tool, name
    from phantom_fhe_amd import pyPhantom as ph
    for name in ("secret_key", "public_key", "batch_encoder"):
        assert not hasattr(ph, name), name
    text = _read("INTEGRATION.md")
    assert "NOT yet in the host mirror" in text and "the cause was not found" in text
