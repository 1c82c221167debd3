"""The samplers and the seeded key generation through the C++ host mirror in the reference's spelling (include/phantom/prng.cuh ->
phantom-fhe_amd/host/phantom.h): tests/cpp/test_prng_spelling.cpp compiles everywhere (CPU check) and, on the GPU box, writes the
words of sample_ternary_poly / sample_error_poly / sample_uniform_poly(_wrap), of the gen_secretkey sequence and of
PhantomRelinKey::generate_seeded / PhantomGaloisKey::generate_seeded on hyb12_a2; they are compared with the restatement
(tests/prng_restatement.py: A of tests/test_gpu_prng.py) and with pha_generate_kswitch_keys_seeded through the C ABI (D)."""
import os
import subprocess

import numpy as np
import pytest

import prng_restatement as R
from util import oracle_ctx, primes_of, rng_for

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_H = [os.path.join(ROOT, "phantom-fhe_amd", "host", "phantom.h"), os.path.join(ROOT, "include", "phantom", "prng.cuh"),
          os.path.join(ROOT, "include", "phantom_amd.h")]
NAME = "hyb12_a2"


def _build():
    import phantom_fhe_amd as P
    src = os.path.join(ROOT, "tests", "cpp", "test_prng_spelling.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "test_prng_spelling")
    libdir = os.path.dirname(P.LIB_PATH)
    newest = max(os.path.getmtime(p) for p in [src] + HOST_H)
    if not os.path.exists(exe) or os.path.getmtime(exe) < newest:
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "include", "phantom"),
                               src, "-o", exe, "-L", libdir, "-lphantom_amd", f"-Wl,-rpath,{libdir}"])
    return exe


def test_prng_spelling_compiles():
    assert os.path.exists(_build())


def test_prng_header_name_resolves_both_ways(tmp_path):
    a = tmp_path / "a.cpp"
    a.write_text('#include "prng.cuh"\nint main() { return random_bytes(3).size() == 3 ? 0 : 1; }\n')
    b = tmp_path / "b.cpp"
    b.write_text("#include <phantom/prng.cuh>\nint main() { return 0; }\n")
    for src, inc in ((a, os.path.join(ROOT, "include", "phantom")), (b, os.path.join(ROOT, "include"))):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-I", inc, str(src)])


@pytest.mark.gpu
def test_mirror_words_equal_the_restatement_and_the_c_abi(gpu, tmp_path):
    import torch
    import phantom_fhe_amd as P
    log_n, primes, size_p = primes_of(NAME)
    primes = [int(q) for q in primes]
    n, size_qp, size_q = 1 << log_n, len(primes), len(primes) - size_p
    dnum = size_q // size_p
    seeds = np.stack([R.seed_bytes(2000 + i) for i in range(20)])
    rng = rng_for(8990)
    new_keys = np.stack([np.stack([rng.integers(0, q, n, dtype=np.uint64) for q in primes[:size_q]]) for _ in range(3)])
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    fin.write_bytes(seeds.tobytes() + new_keys.tobytes())
    run = subprocess.run([_build(), str(fin), str(fout)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "OK" in run.stdout, run.stdout + run.stderr
    words = np.fromfile(str(fout), dtype=np.uint64)
    at = [0]

    def take(*shape):
        count = int(np.prod(shape))
        out = words[at[0]:at[0] + count].reshape(shape)
        at[0] += count
        return out

    # A: the samplers against the restatement
    assert np.array_equal(take(size_qp, n), R.residues(R.ternary_signed(seeds[0], n), primes)), "sample_ternary_poly"
    assert np.array_equal(take(size_qp, n), R.residues(R.error_signed(seeds[0], n), primes)), "sample_error_poly"
    assert np.array_equal(take(size_qp, n), R.uniform(seeds[0], primes, n)), "sample_uniform_poly_wrap"
    assert np.array_equal(take(size_qp - 2, n), R.uniform(seeds[0], primes[2:], n)), "sample_uniform_poly from limb 2"
    # D: the secret key and the keys against the oracle and the C ABI
    sk = take(size_qp, n)
    assert np.array_equal(sk, oracle_ctx(NAME).nwt_forward(R.residues(R.ternary_signed(seeds[1], n), primes), size_qp, 0)), "gen_secretkey"
    ctx = P.PhantomContext(log_n, primes, size_p, device=gpu)
    d_seeds = torch.from_numpy(seeds.copy()).to(gpu)
    d_sk, d_new = P.to_device(sk, gpu), P.to_device(new_keys, gpu)
    relin = ctx.generate_kswitch_keys_seeded(d_sk, d_new[:1], d_seeds[2:2 + 2 * dnum], P.scheme_type.ckks)[0]
    galois = ctx.generate_kswitch_keys_seeded(d_sk, d_new[1:], d_seeds[2 + 2 * dnum:], P.scheme_type.ckks)
    for what, key in (("relin", relin), ("galois 5", galois[0]), ("galois 25", galois[1])):
        for d in range(dnum):
            assert np.array_equal(take(2, size_qp, n), P.to_host(key.public_keys[d])), f"{what} digit {d}"
    assert at[0] == words.size
