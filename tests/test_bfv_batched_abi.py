"""The batched BFV multiply entries exist through every layer (header, library, ctypes table, PhantomContext); no compute, no GPU."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRIES = {
    "pha_bfv_multiply_behz_batched": ("bfv_multiply_behz_batched", ["ct1", "ct2", "dst", "chunk"], 7),
    "pha_bfv_multiply_hps_batched": ("bfv_multiply_hps_batched", ["ct1", "ct2", "dst", "chunk"], 7),
    "pha_bfv_multiply_hps_overq_batched": ("bfv_multiply_hps_overq_batched", ["size_Ql", "ct1", "ct2", "dst", "chunk"], 8),
}


def _header():
    return open(os.path.join(ROOT, "include", "phantom_amd.h")).read()


def test_header_declares_the_batched_entries_as_extensions():
    text = _header()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, (_, _, argc) in ENTRIES.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert m, f"{name} is not declared in include/phantom_amd.h"
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == argc, f"{name}: {args}"
        assert args[0] == "pha_context_t ctx" and args[-1] == "void *stream"
        assert args[-3:-1] == ["size_t batch", "size_t chunk"], f"{name}: {args}"
    # documented like its neighbours: the comment in front of the first declaration says what the reference does instead
    first = min(text.index("int " + name + "(") for name in ENTRIES)
    comment = text[text.rindex("/*", 0, first):first]
    assert "Extension (the reference loops over ciphertexts)" in comment
    assert "[batch][3][Q][N]" in comment and "bit-identical" in comment


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
        assert fn.argtypes[-3] is ctypes.c_size_t and fn.argtypes[-2] is ctypes.c_size_t      # batch, chunk


def test_context_methods_exist_with_a_default_chunk():
    import phantom_fhe_amd as P
    for _, (method, params, _) in ENTRIES.items():
        fn = getattr(P.PhantomContext, method, None)
        assert callable(fn), f"PhantomContext.{method} is missing"
        sig = inspect.signature(fn)
        assert list(sig.parameters)[1:] == params, f"{method}{sig}"
        assert sig.parameters["chunk"].default == 0


def test_no_device_fails_loudly():
    """Without a HIP device there is no context to call the entries on (PhantomContext raises), and the C entries refuse a null
    context with a message instead of computing anything somewhere else."""
    import torch
    import phantom_fhe_amd as P
    from phantom_fhe_amd import lib as L
    lib = L.load()
    for name, (_, _, argc) in ENTRIES.items():
        args = [None] * argc
        args[-3], args[-2] = 1, 0
        if argc == 8:
            args[1] = 1
        assert getattr(lib, name)(*args) == -1, name
        assert b"null context" in lib.pha_last_error()
        with pytest.raises(ValueError):
            L.check(-1)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            P.PhantomContext(12, [0xffffee001, 0xffffc4001, 0x1ffffe0001], 1)
