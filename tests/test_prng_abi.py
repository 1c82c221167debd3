"""The seeded samplers and the seeded key generation exist through the layers that have them (header, library, ctypes table,
PhantomContext, workloads); the host-side pieces (seed derivation, pha_random_bytes) behave as documented.  No GPU."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REF = ["pha_context_t ctx", "uint64_t *out", "const uint8_t *seed", "size_t coeff_mod_size", "size_t mod_start_idx", "void *stream"]
SIGNED = ["pha_context_t ctx", "const uint8_t *seeds", "size_t count", "uint64_t *out", "size_t out_stride", "void *stream"]
# C entry -> (PhantomContext method, its parameters after self, the C argument list of include/phantom_amd.h written out)
ENTRIES = {
    "pha_sample_ternary_poly": ("sample_ternary_poly", ["out", "seed", "coeff_mod_size", "mod_start_idx"], REF),
    "pha_sample_error_poly": ("sample_error_poly", ["out", "seed", "coeff_mod_size", "mod_start_idx"], REF),
    "pha_sample_uniform_poly": ("sample_uniform_poly", ["out", "seed", "coeff_mod_size", "mod_start_idx"], REF),
    "pha_sample_ternary_signed_batched": ("sample_ternary_signed_batched", ["seeds", "out", "count", "out_stride"], SIGNED),
    "pha_sample_error_signed_batched": ("sample_error_signed_batched", ["seeds", "out", "count", "out_stride"], SIGNED),
    "pha_sample_uniform_batched": (
        "sample_uniform_batched", ["size_Ql", "seeds", "out", "with_special", "count", "out_stride"],
        ["pha_context_t ctx", "size_t size_Ql", "int with_special", "const uint8_t *seeds", "size_t count", "uint64_t *out",
         "size_t out_stride", "void *stream"]),
    "pha_secret_key_generate": (
        "secret_key_generate", ["seed", "sk_ntt"], ["pha_context_t ctx", "const uint8_t *seed", "uint64_t *sk_ntt", "void *stream"]),
    "pha_generate_kswitch_keys_seeded": (
        "generate_kswitch_keys_seeded", ["sk_ntt", "new_keys_ntt", "seeds", "scheme", "evk"],
        ["pha_context_t ctx", "const uint64_t *sk_ntt", "const uint64_t *new_keys_ntt", "size_t n_keys", "size_t new_key_stride",
         "const uint8_t *seeds", "uint64_t *evk", "size_t evk_stride", "int scheme", "void *stream"]),
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
    assert re.search(r"\bint\s+pha_random_bytes\s*\(\s*unsigned char \*host_buf,\s*size_t count\s*\)\s*;", code)
    first = text.index("int pha_random_bytes(")
    comment = text[text.rindex("/*", 0, first):first]
    for name in list(ENTRIES) + ["pha_random_bytes"]:
        assert name in comment, f"{name} is not described in the section's comment"
    for word in ("src/prng.cu", "src/secretkey.cu:297-460", "64 bytes", "bytes 56..63 are never", "WITHOUT constants", "ONE block per coefficient",
                 "tries * N * cms", "SIGNED 64-bit words", "POSITION", "a is never copied", "[n_keys][dnum][2][64]", "gen_relinkey",
                 "create_galois_keys", "ONE pha_encrypt_zero_symmetric_batched", "Word for word", "std::random_device", "count == 0",
                 "16-byte", "can be captured into a graph", "only pha_random_bytes draws entropy", "src/secretkey.cu:46-55, 80-81",
                 "equal seeds reproduce the reference"):
        assert word in comment, word
    # the sections that used to say the library draws no random number now point here
    assert "is outside the accelerated path" not in text
    assert "the PRNG (src/prng.cu) is not part of this library" not in text


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
    assert hasattr(so, "pha_random_bytes") and "pha_random_bytes" in P.EXPORTED


def test_context_methods_and_workloads_exist():
    import phantom_fhe_amd as P
    from phantom_fhe_amd import workloads as W
    for name, (method, params, _) in ENTRIES.items():
        fn = getattr(P.PhantomContext, method, None)
        assert callable(fn), f"PhantomContext.{method} is missing"
        assert list(inspect.signature(fn).parameters)[1:] == params, f"{method}{inspect.signature(fn)}"
    assert list(inspect.signature(W.derive_seeds).parameters) == ["master", "label", "count"]
    sig = inspect.signature(W.keygen)
    assert list(sig.parameters) == ["ctx", "scheme", "galois_elts", "master", "max_power"]
    assert sig.parameters["galois_elts"].default == () and sig.parameters["master"].default is None and sig.parameters["max_power"].default == 2
    sig = inspect.signature(W.sample_encryption)
    assert list(sig.parameters) == ["ctx", "level", "count", "master", "public"] and sig.parameters["public"].default is False
    # the existing compositions keep their signatures
    assert list(inspect.signature(W.encode_encrypt_batch).parameters) == ["ctx", "encoder", "messages", "level", "scale", "key", "samples", "public"]
    assert list(inspect.signature(W.batch_encode_encrypt).parameters) == ["ctx", "encoder", "messages", "level", "key", "samples", "scheme", "public"]


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


def test_derive_seeds_is_deterministic_and_separated():
    import hashlib
    from phantom_fhe_amd import workloads as W
    master = bytes(range(64))
    a = W.derive_seeds(master, "ksk", 5)
    assert a.shape == (5, 64) and a.dtype == np.uint8
    assert np.array_equal(a, W.derive_seeds(master, "ksk", 5))                    # deterministic
    assert np.array_equal(a[:3], W.derive_seeds(master, "ksk", 3))                # seed i does not depend on the count
    assert bytes(a[2]) == hashlib.blake2b(master + b"ksk" + (2).to_bytes(8, "little"), digest_size=64).digest()
    assert len({bytes(r) for r in a}) == 5                                         # counter-separated
    b = W.derive_seeds(master, "pk", 5)
    assert not any(bytes(x) == bytes(y) for x in a for y in b)                     # label-separated
    assert not np.array_equal(a, W.derive_seeds(bytes(range(1, 65)), "ksk", 5))   # master-separated
    assert np.array_equal(W.derive_seeds(master, b"ksk", 1), a[:1])               # a bytes label is taken as it is
    fresh = W.derive_seeds(None, "sk", 1), W.derive_seeds(None, "sk", 1)           # master=None: fresh entropy each time
    assert fresh[0].shape == (1, 64) and not np.array_equal(*fresh)
    assert W.derive_seeds(master, "sk", 0).shape == (0, 64)


def test_random_bytes_fills_count_bytes_and_two_calls_differ():
    import phantom_fhe_amd as P
    from phantom_fhe_amd import lib as L
    lib = L.load()
    for count in (0, 1, 3, 64, 67):
        buf = (ctypes.c_ubyte * (count + 8))(*([0xA5] * (count + 8)))
        assert lib.pha_random_bytes(buf, count) == 0
        assert list(buf[count:]) == [0xA5] * 8, f"count {count}: bytes past the end were written"
    a, b = P.random_bytes(64), P.random_bytes(64)
    assert len(a) == 64 and len(b) == 64 and a != b
    assert len(set(P.random_bytes(4096))) > 200                                    # every byte of the buffer is filled, not just a prefix
    assert lib.pha_random_bytes(None, 4) == -1 and b"null" in lib.pha_last_error()
    assert lib.pha_random_bytes(None, 0) == 0


def test_the_documents_no_longer_say_the_library_draws_no_random_number():
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        text = _read(doc)
        assert "pha_sample_uniform_batched" in text and "pha_generate_kswitch_keys_seeded" in text, doc
    design = _read("DESIGN.md")
    assert "4.14" in design and "pha_prng.h" in design
    integ = _read("INTEGRATION.md")
    for word in ("only `pha_random_bytes` draws entropy", "src/secretkey.cu:46-55", "PhantomSecretKey", "PhantomPublicKey"):
        assert word in integ, word
