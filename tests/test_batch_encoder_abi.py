"""The BFV / BGV batch encoder exists through the layers that have it (header, library, ctypes table, BatchEncoder, workloads); no
compute, no GPU."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# C entry -> (BatchEncoder method or None, its parameters after self, the C argument list of include/phantom_amd.h written out)
ENTRIES = {
    "pha_batch_encoder_create": (None, None, ["pha_context_t ctx", "pha_batch_encoder_t *enc"]),
    "pha_batch_encoder_index_map": ("index_map", [], ["pha_batch_encoder_t enc", "uint64_t *index_map_host"]),
    "pha_plain_nwt_forward_inplace_batched": (
        "plain_nwt_forward_inplace_batched", ["inout", "count", "stride"],
        ["pha_batch_encoder_t enc", "uint64_t *inout", "size_t count", "size_t stride", "void *stream"]),
    "pha_plain_nwt_backward_inplace_batched": (
        "plain_nwt_backward_inplace_batched", ["inout", "count", "stride"],
        ["pha_batch_encoder_t enc", "uint64_t *inout", "size_t count", "size_t stride", "void *stream"]),
    "pha_batch_encode_batched": (
        "encode_batched", ["values", "values_size", "dst", "count", "strides"],
        ["pha_batch_encoder_t enc", "const uint64_t *values", "size_t values_size", "size_t count", "size_t values_stride", "uint64_t *dst",
         "size_t dst_stride", "void *stream"]),
    "pha_batch_decode_batched": (
        "decode_batched", ["plain", "values_out", "count", "strides"],
        ["pha_batch_encoder_t enc", "const uint64_t *plain", "size_t count", "size_t plain_stride", "uint64_t *values_out",
         "size_t values_stride", "void *stream"]),
}
TAKE_ENCODER = [n for n in ENTRIES if n != "pha_batch_encoder_create"]


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_header_declares_and_documents_the_seven_entries():
    text = _read("include", "phantom_amd.h")
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"typedef\s+struct\s+pha_batch_encoder\s*\*\s*pha_batch_encoder_t\s*;", code)
    assert re.search(r"\bvoid\s+pha_batch_encoder_destroy\s*\(\s*pha_batch_encoder_t\s+enc\s*\)\s*;", code)
    for name, (_, _, want) in ENTRIES.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert m, f"{name} is not declared in include/phantom_amd.h"
        args = [" ".join(a.split()) for a in m.group(1).split(",")]
        assert args == want, f"{name}: {args}"
    first = text.index("typedef struct pha_batch_encoder ")
    assert first > text.index("int pha_encrypt_asymmetric_batched(")          # a new section after the encryption section
    comment = text[text.rindex("/*", 0, first):first]
    flat = " ".join(comment.replace("\n *", " ").split())                       # the comment as running text
    for name in list(ENTRIES):
        base = name.replace("_backward_", "_forward_")                         # the two transforms are described as "_forward_ / _backward_"
        assert base in flat, f"{name} is not described in the section's comment"
    for word in ("src/batchencoder.cu:7-118", ":7-49", ":51-89", ":91-118", "gpu_plain_tables()", "matrix_reps_index_map", "minimal primitive",
                 "bit 63 set gets + t", "values_stride == 0 shares", "values_size == 0 encodes zeros", "count == 0 is a no-op",
                 "values_matrix size is too large", "encryption parameters are not valid for batching", "null encoder", "has changed since",
                 "must outlive", "no caller-supplied word becomes an address", "outputs are below t", "captured into a graph",
                 "PHA_STRICT: <entry> values holds k word(s)", "<entry> plain", "gains no row"):
        assert word in flat, word
    strict = text[text.index("pha_set_strict(on)"):text.index("int pha_check_canonical(")]
    for name in ("pha_batch_encode_batched", "pha_batch_decode_batched"):
        assert name in strict, f"{name} is missing from the strict-mode list"
    bench = _read("include", "phantom_amd_bench.h")
    for hook in ("pha_batch_set_encode_path", "pha_batch_set_decode_path"):
        assert re.search(r"\bint\s+" + hook + r"\s*\(\s*int\s+mode\s*\)\s*;", bench), hook


def test_library_exports_and_binding_declares_them():
    import phantom_fhe_amd as P
    from phantom_fhe_amd import lib as L
    if not os.path.exists(P.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    so = ctypes.CDLL(P.LIB_PATH)
    for name in list(ENTRIES) + ["pha_batch_encoder_destroy", "pha_batch_set_encode_path", "pha_batch_set_decode_path"]:
        assert hasattr(so, name), f"{name} is not exported by the built library"
        assert name in P.EXPORTED, f"{name} has no argtypes in phantom_fhe_amd/lib.py"
    for name, (_, _, want) in ENTRIES.items():
        fn = getattr(L.load(), name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(want), f"{name}: {fn.argtypes}"
        for t, decl in zip(fn.argtypes, want):
            if decl.startswith("size_t"):
                assert t is ctypes.c_size_t, f"{name}: {decl} bound as {t}"
            else:                                                              # handles, device pointers, host arrays: pointers all
                assert t is ctypes.c_void_p or issubclass(t, ctypes._Pointer), f"{name}: {decl} bound as {t}"
    assert L.load().pha_batch_encoder_destroy.restype is None


def test_encoder_class_and_workloads_exist():
    import phantom_fhe_amd as P
    from phantom_fhe_amd import workloads as W
    assert list(inspect.signature(P.BatchEncoder.__init__).parameters) == ["self", "ctx"]
    for name, (method, params, _) in ENTRIES.items():
        if method is None:
            continue
        fn = getattr(P.BatchEncoder, method, None)
        assert callable(fn), f"BatchEncoder.{method} is missing"
        sig = inspect.signature(fn)
        assert list(sig.parameters)[1:] == params, f"{method}{sig}"
        for opt in ("count", "stride", "strides"):
            if opt in params:
                assert sig.parameters[opt].default is None
    sig = inspect.signature(W.batch_encode_encrypt)
    assert list(sig.parameters) == ["ctx", "encoder", "messages", "level", "key", "samples", "scheme", "public"]
    assert sig.parameters["public"].default is False
    sig = inspect.signature(W.batch_decrypt_decode)
    assert list(sig.parameters) == ["ctx", "encoder", "cts", "level", "sk_powers", "scheme", "correction_factors"]
    assert sig.parameters["correction_factors"].default is None
    assert callable(P.set_batch_encode_path) and callable(P.set_batch_decode_path)


def test_null_encoder_and_null_context_are_refused_with_a_message():
    from phantom_fhe_amd import lib as L
    lib = L.load()
    for name in TAKE_ENCODER:
        fn = getattr(lib, name)
        args = [1 if t is ctypes.c_size_t else None for t in fn.argtypes]
        assert fn(*args) == -1, name
        assert b"null encoder" in lib.pha_last_error()
        with pytest.raises(ValueError):
            L.check(-1)
    assert lib.pha_batch_encoder_create(None, None) == -1
    assert b"null context" in lib.pha_last_error()
    lib.pha_batch_encoder_destroy(None)                                        # like free(): nothing happens


def test_what_stays_absent_is_stated():
    """The encoder stops where decryption and encryption stop: the C ABI, phantom_fhe_amd, workloads.  The PRNG and the key and
    encoder classes of the host mirror / pyPhantom stay absent."""
    host = _read("phantom-fhe_amd", "host", "phantom.h")
    assert "class PhantomBatchEncoder" not in host and "class PhantomSecretKey" not in host
    from phantom_fhe_amd import pyPhantom as ph
    for name in ("batch_encoder", "secret_key", "public_key"):
        assert not hasattr(ph, name), name
    text = _read("INTEGRATION.md")
    for word in ("pha_batch_encode_batched", "pha_batch_decode_batched", "pha_plain_nwt_forward_inplace_batched", "PhantomBatchEncoder::encode",
                 "gpu_plain_tables()", "src/prng.cu", "NOT yet in the host mirror"):
        assert word in text, word
    for doc in ("README.md", "DESIGN.md"):
        assert "pha_batch.hip" in _read(doc), doc
    assert "4.13" in _read("DESIGN.md")
