"""The CKKS encoder exists through every layer (header, library, ctypes table, PhantomContext / CKKSEncoder, host mirror header,
pyPhantom.ckks_encoder, workloads); no compute, no GPU."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# C entry -> the C argument list of include/phantom_amd.h written out
ENTRIES = {
    "pha_ckks_encoder_create": ["pha_context_t ctx", "pha_ckks_encoder_t *enc"],
    "pha_ckks_encoder_tables": ["pha_ckks_encoder_t enc", "double *roots_host", "uint32_t *group_host"],
    "pha_special_fft_backward": ["pha_ckks_encoder_t enc", "double *inout", "size_t log_n", "double scalar", "void *stream"],
    "pha_special_fft_forward": ["pha_ckks_encoder_t enc", "double *inout", "size_t log_n", "void *stream"],
    "pha_decompose_array": ["pha_context_t ctx", "size_t size_Ql", "uint64_t *dst", "const double *src", "uint32_t max_coeff_bit_count",
                            "void *stream"],
    "pha_compose_array": ["pha_context_t ctx", "size_t size_Ql", "double *dst", "const uint64_t *src", "double inv_scale", "void *stream"],
    "pha_ckks_encode_batched": ["pha_ckks_encoder_t enc", "size_t size_Ql", "int with_special", "const double *values", "size_t values_size",
                                "size_t count", "size_t values_stride", "double scale", "uint64_t *dst", "size_t dst_stride",
                                "int *bit_counts_host_or_null", "void *stream"],
    "pha_ckks_decode_batched": ["pha_ckks_encoder_t enc", "size_t size_Ql", "const uint64_t *plain", "size_t count", "size_t plain_stride",
                                "double scale", "double *values_out", "size_t values_stride", "void *stream"],
}


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_header_declares_and_documents_the_entries():
    text = _read("include", "phantom_amd.h")
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, want in ENTRIES.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert m, f"{name} is not declared in include/phantom_amd.h"
        assert [" ".join(a.split()) for a in m.group(1).split(",")] == want, name
    assert re.search(r"\bvoid\s+pha_ckks_encoder_destroy\s*\(\s*pha_ckks_encoder_t enc\s*\)\s*;", code)
    first = text.index("typedef struct pha_ckks_encoder *pha_ckks_encoder_t;")
    comment = text[text.rindex("/*", 0, first):first]
    for needle in ("SYNCHRONISES", "values_stride counts complex numbers", "Strict mode checks plain", "-0.0", "arenas",
                   "ar*br - ai*bi", "encoded values are too large", "[0, size_Ql) u P"):
        assert needle in comment, needle


def test_arithmetic_header_states_the_no_contraction_rule():
    text = _read("phantom-fhe_amd", "csrc", "pha_ckks_fft.h")
    assert "#pragma clang fp contract(off)" in text and "PHA_HD" in text
    assert "pha_ckks_fft.h" in _read("tests", "emu", "emu_ckks_fft.cpp")       # the harness compiles the kernels' source


def test_library_exports_and_binding_declares_them():
    import phantom_fhe_amd as P
    from phantom_fhe_amd import lib as L
    if not os.path.exists(P.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    so = ctypes.CDLL(P.LIB_PATH)
    for name, want in list(ENTRIES.items()) + [("pha_ckks_encoder_destroy", ["pha_ckks_encoder_t enc"])]:
        assert hasattr(so, name), f"{name} is not exported by the built library"
        assert name in P.EXPORTED, f"{name} has no argtypes in phantom_fhe_amd/lib.py"
        fn = getattr(L.load(), name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(want), f"{name}: {fn.argtypes}"
        for t, decl in zip(fn.argtypes, want):
            kind = None if "*" in decl or decl.startswith("pha_") else decl.split()[0]
            expect = {"size_t": ctypes.c_size_t, "int": ctypes.c_int, "double": ctypes.c_double, "uint32_t": ctypes.c_uint32, None: None}[kind]
            if expect is not None:
                assert t is expect, f"{name}: {decl} bound as {t}"
            else:
                assert t not in (ctypes.c_size_t, ctypes.c_int, ctypes.c_double, ctypes.c_uint32), f"{name}: {decl} bound as {t}"


def test_python_layers_have_the_methods():
    import phantom_fhe_amd as P
    from phantom_fhe_amd import workloads as W
    for method in ("decompose_array", "compose_array", "ckks_encoder"):
        assert callable(getattr(P.PhantomContext, method, None)), method
    for method in ("tables", "special_fft_backward", "special_fft_forward", "encode_batched", "decode_batched"):
        assert callable(getattr(P.CKKSEncoder, method, None)), method
    sig = inspect.signature(P.CKKSEncoder.encode_batched)
    assert list(sig.parameters)[1:] == ["size_Ql", "values", "values_size", "scale", "dst", "with_special", "count", "strides"]
    assert sig.parameters["with_special"].default is False
    assert list(inspect.signature(W.encode_diagonals).parameters) == ["encoder", "size_Ql", "matrix", "scale", "steps"]
    m = np.arange(16).reshape(4, 4)
    d = W.matrix_diagonals(m, 8)
    assert d.shape == (4, 8) and d[0].real.tolist() == [0, 5, 10, 15] * 2 and d[1].real.tolist() == [1, 6, 11, 12] * 2
    v = np.arange(1, 5)
    assert np.allclose(sum(d[k][:4] * np.roll(v, -k) for k in range(4)), m @ v)
    with pytest.raises(ValueError):
        W.matrix_diagonals(np.zeros((3, 3)), 8)


def test_pyphantom_has_the_reference_names():
    from phantom_fhe_amd import pyPhantom as ph
    assert hasattr(ph, "ckks_encoder")
    for name in ("slot_count", "encode_complex_vector", "encode_double_vector", "decode_complex_vector", "decode_double_vector"):
        assert hasattr(ph.ckks_encoder, name), name
    assert "chain_index" in ph.ckks_encoder.encode_double_vector.__doc__
    assert "PhantomCKKSEncoder" in _read("phantom-fhe_amd", "host", "phantom.h")
    assert "phantom.h" in _read("include", "phantom", "ckks.h")


def test_null_handles_are_refused_with_a_message():
    from phantom_fhe_amd import lib as L
    lib = L.load()
    for name in ENTRIES:
        fn = getattr(lib, name)
        args = [None if t not in (ctypes.c_size_t, ctypes.c_int, ctypes.c_double, ctypes.c_uint32) else 1 for t in fn.argtypes]
        assert fn(*args) == -1, name
        assert b"null" in lib.pha_last_error()
    lib.pha_ckks_encoder_destroy(None)
    with pytest.raises(ValueError):
        L.check(-1)
