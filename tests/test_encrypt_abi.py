"""The encryption entries exist through the layers that have them (header, library, ctypes table, PhantomContext, workloads);
no compute, no GPU."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# C entry -> (PhantomContext method, its parameters after self, the C argument list of include/phantom_amd.h written out)
ENTRIES = {
    "pha_encrypt_zero_symmetric_batched": (
        "encrypt_zero_symmetric_batched", ["size_Ql", "sk_ntt", "e", "ct", "scheme", "with_special", "ntt_form", "count", "strides"],
        ["pha_context_t ctx", "size_t size_Ql", "int with_special", "const uint64_t *sk_ntt", "const uint64_t *e", "size_t e_stride",
         "uint64_t *ct", "size_t ct_stride", "size_t count", "int scheme", "int ntt_form", "void *stream"]),
    "pha_public_key_generate": (
        "public_key_generate", ["sk_ntt", "e", "pk", "scheme"],
        ["pha_context_t ctx", "const uint64_t *sk_ntt", "const uint64_t *e", "uint64_t *pk", "int scheme", "void *stream"]),
    "pha_encrypt_symmetric_batched": (
        "encrypt_symmetric_batched", ["size_Ql", "sk_ntt", "e", "plain", "ct", "scheme", "count", "strides"],
        ["pha_context_t ctx", "size_t size_Ql", "const uint64_t *sk_ntt", "const uint64_t *e", "size_t e_stride", "const uint64_t *plain",
         "size_t plain_stride", "uint64_t *ct", "size_t ct_stride", "size_t count", "int scheme", "void *stream"]),
    "pha_encrypt_asymmetric_batched": (
        "encrypt_asymmetric_batched", ["size_Ql", "pk", "u", "e", "plain", "ct", "scheme", "count", "strides", "chunk"],
        ["pha_context_t ctx", "size_t size_Ql", "const uint64_t *pk", "const uint64_t *u", "size_t u_stride", "const uint64_t *e",
         "size_t e_stride", "const uint64_t *plain", "size_t plain_stride", "uint64_t *ct", "size_t ct_stride", "size_t count", "int scheme",
         "size_t chunk", "void *stream"]),
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
    first = text.index("int pha_encrypt_zero_symmetric_batched(")
    comment = text[text.rindex("/*", 0, first):first]
    for name in ENTRIES:
        assert name in comment, f"{name} is not described in the section's comment"
    for word in ("src/secretkey.cu:11-192", "gen_publickey", "SIGNED 64-bit words", "|v| <= 2^16", "below 2^17", "ALREADY in c1's place",
                 "with_special", "[2][size_QP][N]", "plain_stride 0 shares", "DRNSTool::moddown", "src/secretkey.cu:106-121", "Extension",
                 "Every `chunk` gives", "count == 0", "can be captured into a graph", "<entry> sk", "<entry> pk", "<entry> a", "<entry> plain",
                 "<entry> samples", "src/prng.cu"):
        assert word in comment, word
    strict = text[text.index("pha_set_strict(on)"):text.index("int pha_check_canonical(")]
    for name in ENTRIES:
        assert name in strict, f"{name} is missing from the strict-mode list"
    decrypt = text[text.index("/* ---- decryption"):text.index("int pha_secret_key_powers(")]
    assert "encryption\n *      and public keys are not part of this library" not in decrypt
    assert "not part of this library" in decrypt and "src/prng.cu" in decrypt      # what stays absent: sampling


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
    sig = inspect.signature(W.encode_encrypt_batch)
    assert list(sig.parameters) == ["ctx", "encoder", "messages", "level", "scale", "key", "samples", "public"]
    assert sig.parameters["public"].default is False


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


def test_what_stays_absent_is_stated():
    """encryption stops at the C ABI and phantom_fhe_amd; the PRNG, the BFV / BGV batch encoder and the secret-key
    classes of the host mirror / pyPhantom stay absent."""
    host = _read("phantom-fhe_amd", "host", "phantom.h")
    assert "class PhantomSecretKey" not in host and "class PhantomPublicKey" not in host
    from phantom_fhe_amd import pyPhantom as ph
    for name in ("secret_key", "public_key", "batch_encoder"):
        assert not hasattr(ph, name), name
    text = _read("INTEGRATION.md")
    for word in ("pha_encrypt_symmetric_batched", "pha_encrypt_asymmetric_batched", "pha_public_key_generate", "src/prng.cu",
                 "NOT yet in the host mirror", "the cause was not found"):
        assert word in text, word
