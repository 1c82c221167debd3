"""Seeded samplers and seeded key generation on the GPU (csrc/pha_prng.hip), word for word against tests/prng_restatement.py:

A. the three reference-layout launchers (pha_sample_ternary_poly / _error_poly / _uniform_poly) on hyb12_a2 (8 limbs, 40 / 60 bits),
   ladder12 (every width of the reduction), reject12 (5.88 % of the words are redrawn; the fixed seed whose redraw log
   tests/test_prng_restatement.py pins) and hyb17_a2 (N = 2^17: nonces and group indexes past 2^16), with mod_start_idx 0 and 2;
B. the compact batched forms on hyb12_a2, count 1, 5, 9, padded stride: out (b) is the restatement for seed b, and lifted modulo each
   prime it is what A's launchers write;
C. pha_sample_uniform_batched on hyb12_a2 at levels 6 and 3, with and without the special rows, count 1 and 5, into c1's place of a
   [count][2][rows][N] buffer (c0 untouched); at level 6 with the special rows it is A's pha_sample_uniform_poly over QP; the same
   on reject12;
D. key generation on hyb12_a2 and hyb13_a3, ckks and bgv: the secret key is the oracle's forward transform of the restated ternary
   sample; pha_generate_kswitch_keys_seeded with 1 and 3 keys is pha_generate_one_kswitch_key per key on the restated a and the
   restated noise expanded to residues;
E. round trips with nothing made on the host but the master seed: keygen -> sample_encryption -> encode + encrypt (symmetric and
   public) -> product, relinearisation (+ rescale), one rotation through the generated Galois key -> decrypt + decode, against numpy
   on the slots; ckks within the bound of tests/test_gpu_ckks_semantics.py (16 x the oracle pipeline's error on the same messages,
   capped at 2^-12), bgv and bfv exact at t = 65537; the same master gives the same words twice, another master other keys;
F. refusals with nothing launched, count == 0, one key generation captured into a graph (one stream) and replayed.
Outputs are poisoned first; strided padding and the inputs are checked untouched."""
import functools
import gc

import numpy as np
import pytest

import ckks_semantics as S
import prng_restatement as R
from oracle import oracle as O
from util import first_diff_limb, oracle_ctx, primes_of, rng_for

pytestmark = pytest.mark.gpu

POISON = -0x2152411021524111
POISON_U = np.uint64(POISON & (2 ** 64 - 1))
T = 65537
PAD = 6          # words between strided results (strides stay even)


def _release():
    import torch
    gc.collect()
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def _params(name):
    log_n, primes, size_p = R.REJECT12 if name == "reject12" else primes_of(name)
    return log_n, tuple(int(q) for q in primes), size_p


def _ctx(name, gpu, plain_t=0):
    import phantom_fhe_amd as P
    log_n, primes, size_p = _params(name)
    ctx = P.PhantomContext(log_n, list(primes), size_p, device=gpu)
    if plain_t:
        ctx.set_plain_modulus(plain_t)
    return P, ctx


def _poisoned(shape, gpu):
    import torch
    return torch.full(shape, POISON, dtype=torch.int64, device=gpu)


def _seed_of(name, tag):
    return np.ascontiguousarray(R.STAT_SEED_ARRAY if name == "reject12" and tag == 0 else R.seed_bytes(1000 + tag))


def _dseeds(seeds, gpu):
    import torch
    return torch.from_numpy(np.array(seeds, dtype=np.uint8)).to(gpu)     # a copy: the fixed seed's array is read-only


@functools.lru_cache(maxsize=None)
def _signed_ref(name, kind, tag):
    """The restated ternary / noise sample of (set, seed tag): [N] int64.  Computed once."""
    n = 1 << _params(name)[0]
    out = (R.ternary_signed if kind == "ternary" else R.error_signed)(_seed_of(name, tag), n)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _uniform_ref(name, tag, rows):
    """The restated uniform sample of (set, seed tag) over the prime-table rows `rows` (a tuple, in buffer order)."""
    log_n, primes, _ = _params(name)
    out = R.uniform(_seed_of(name, tag), [primes[r] for r in rows], 1 << log_n)
    out.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# A: the reference-layout launchers
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mod_start", [0, 2])
@pytest.mark.parametrize("name", ["hyb12_a2", "ladder12", "reject12", "hyb17_a2"])
def test_reference_layout_launchers_word_for_word(name, mod_start, gpu):
    P, ctx = _ctx(name, gpu)
    log_n, primes, _ = _params(name)
    n, rows = 1 << log_n, tuple(range(mod_start, len(primes)))
    cms, used = len(rows), [primes[r] for r in rows]
    seed = _dseeds(_seed_of(name, 0), gpu)
    want = {"ternary": R.residues(_signed_ref(name, "ternary", 0), used), "error": R.residues(_signed_ref(name, "error", 0), used),
            "uniform": _uniform_ref(name, 0, rows)}
    for kind, fn in (("ternary", ctx.sample_ternary_poly), ("error", ctx.sample_error_poly), ("uniform", ctx.sample_uniform_poly)):
        out = _poisoned((cms * n + PAD,), gpu)
        fn(out, seed, cms, mod_start)
        got = P.to_host(out)
        first_diff_limb(got[:cms * n].reshape(cms, n), want[kind], f"{kind} {name} mod_start {mod_start}", used)
        assert np.all(got[cms * n:] == POISON_U), f"{kind}: words past the polynomial were written"
    assert np.array_equal(seed.cpu().numpy(), _seed_of(name, 0)), "the seed was written to"
    if name == "reject12":                                     # the inputs do redraw (the log itself: tests/test_prng_restatement.py)
        log = []
        R.uniform(_seed_of(name, 0), used, n, log)
        assert len(log) >= 100 * cms and any(r >= 2 for _, _, _, r in log)
    del ctx
    _release()


# ------------------------------------------------------------------------------------------------------------------------------
# B: the compact signed forms
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 5, 9])
def test_signed_batched_forms(count, gpu):
    name = "hyb12_a2"
    P, ctx = _ctx(name, gpu)
    log_n, primes, _ = _params(name)
    n, stride = 1 << log_n, (1 << log_n) + PAD
    seeds = np.stack([_seed_of(name, b) for b in range(count)])
    d_seeds = _dseeds(seeds, gpu)
    for kind, batched, single in (("ternary", ctx.sample_ternary_signed_batched, ctx.sample_ternary_poly),
                                  ("error", ctx.sample_error_signed_batched, ctx.sample_error_poly)):
        out = _poisoned((count * stride,), gpu)
        batched(d_seeds, out, count=count, out_stride=stride)
        got = P.to_host(out).reshape(count, stride)
        assert np.all(got[:, n:] == POISON_U), f"{kind}: the padding between the polynomials was written to"
        for b in range(count):
            v = got[b, :n].view(np.int64)
            assert np.array_equal(v, _signed_ref(name, kind, b)), f"{kind} count {count}: out({b}) differs from the restatement"
            res = _poisoned((len(primes), n), gpu)
            single(res, d_seeds[b], len(primes), 0)
            first_diff_limb(R.residues(v, primes), P.to_host(res), f"{kind} seed {b}: the signed form lifted against the residue form", primes)
    assert np.array_equal(d_seeds.cpu().numpy(), seeds)
    del ctx
    _release()


# ------------------------------------------------------------------------------------------------------------------------------
# C: the uniform sampler into c1's place
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,level", [("hyb12_a2", 6), ("hyb12_a2", 3), ("reject12", 2), ("reject12", 1)])
@pytest.mark.parametrize("special", [False, True], ids=["data", "special"])
def test_uniform_batched_into_c1(name, level, special, gpu):
    P, ctx = _ctx(name, gpu)
    log_n, primes, size_p = _params(name)
    n, size_q = 1 << log_n, len(primes) - size_p
    rows = tuple(range(level)) + (tuple(range(size_q, len(primes))) if special else ())
    used = [primes[r] for r in rows]
    for count in (1, 5):
        seeds = np.stack([_seed_of(name, b) for b in range(count)])
        d_seeds = _dseeds(seeds, gpu)
        ct = _poisoned((count, 2, len(rows), n), gpu)
        ctx.sample_uniform_batched(level, d_seeds, ct[:, 1], with_special=special)
        got = P.to_host(ct)
        assert np.all(got[:, 0] == POISON_U), "c0 was written to"
        for b in range(count):
            first_diff_limb(got[b, 1], _uniform_ref(name, b, rows), f"uniform {name} level {level} special {special} count {count} b {b}", used)
        if level == size_q and special:                        # the reference's sample_uniform_poly over QP
            ref = _poisoned((len(primes), n), gpu)
            ctx.sample_uniform_poly(ref, d_seeds[0], len(primes), 0)
            assert np.array_equal(got[0, 1], P.to_host(ref))
        assert np.array_equal(d_seeds.cpu().numpy(), seeds)
    del ctx
    _release()


# ------------------------------------------------------------------------------------------------------------------------------
# D: key generation
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", [O.CKKS, O.BGV], ids=["ckks", "bgv"])
@pytest.mark.parametrize("name", ["hyb12_a2", "hyb13_a3"])
def test_key_generation_word_for_word(name, scheme, gpu):
    P, ctx = _ctx(name, gpu, 0 if scheme == O.CKKS else T)
    kind = P.scheme_type.ckks if scheme == O.CKKS else P.scheme_type.bgv
    log_n, primes, size_p = _params(name)
    n, size_qp, size_q = 1 << log_n, len(primes), len(primes) - size_p
    dnum, oc = size_q // size_p, oracle_ctx(name)
    # the secret key
    sk = _poisoned((size_qp, n), gpu)
    seed = _dseeds(_seed_of(name, 40), gpu)
    assert ctx.secret_key_generate(seed, sk) is sk
    want_sk = oc.nwt_forward(R.residues(_signed_ref(name, "ternary", 40), primes), size_qp, 0)
    first_diff_limb(P.to_host(sk), want_sk, f"secret key {name}", primes)
    # the key-switching keys
    rng = rng_for(8800 + log_n)
    for n_keys in (1, 3):
        new_keys = np.stack([np.stack([rng.integers(0, q, n, dtype=np.uint64) for q in primes[:size_q]]) for _ in range(n_keys)])
        tags = np.arange(50, 50 + 2 * n_keys * dnum).reshape(n_keys, dnum, 2)
        seeds = np.stack([_seed_of(name, int(t)) for t in tags.reshape(-1)]).reshape(n_keys, dnum, 2, 64)
        d_new, d_seeds = P.to_device(new_keys, gpu), _dseeds(seeds, gpu)
        evk = _poisoned((n_keys, dnum, 2, size_qp, n), gpu)
        keys = ctx.generate_kswitch_keys_seeded(sk, d_new, d_seeds, kind, evk=evk)
        assert len(keys) == n_keys and all(len(k.public_keys) == dnum for k in keys)
        got = P.to_host(evk)
        for k in range(n_keys):
            a = np.stack([_uniform_ref(name, int(tags[k, d, 0]), tuple(range(size_qp))) for d in range(dnum)])
            e = np.stack([R.residues(_signed_ref(name, "error", int(tags[k, d, 1])), primes) for d in range(dnum)])
            ref = ctx.generate_one_kswitch_key(sk, d_new[k], P.to_device(a, gpu), P.to_device(e, gpu), kind)
            for d in range(dnum):
                first_diff_limb(got[k, d], P.to_host(ref.public_keys[d]), f"{name} scheme {scheme} n_keys {n_keys} key {k} digit {d}", primes)
                assert keys[k].public_keys[d].data_ptr() == evk[k, d].data_ptr()           # the tables point into the storage: no copy
        assert np.array_equal(P.to_host(d_new), new_keys) and np.array_equal(d_seeds.cpu().numpy(), seeds)
    assert np.array_equal(P.to_host(sk), want_sk), "the secret key was written to"
    del ctx
    _release()


# ------------------------------------------------------------------------------------------------------------------------------
# E: round trips from a master seed
# ------------------------------------------------------------------------------------------------------------------------------
MASTER = bytes((7 * i + 3) & 0xFF for i in range(64))


@functools.lru_cache(maxsize=None)
def _cpu_product_then_rotation(level, scale, step):
    """The oracle pipeline on the same messages with the helper's own keys and encryption: the baseline of the bound."""
    sch, codec = S.scheme("hyb12_a2"), S.cpu_codec("hyb12_a2")
    ref = S.Reference(sch, codec)
    z = S.messages(12, 2, sch.slots)
    a, b = (S._enc(sch, codec, z[k:k + 1], level, scale, f"prng.{k}")[0] for k in range(2))
    prod = ref.multiply_many([a], [b], level)[0]
    rot = ref.rotate(prod, level - 1, S.elt_of_step(step, sch.n))
    out_scale = scale * scale / float(sch.primes[level - 1])
    return S.max_err(S._dec(sch, codec, [rot], level - 1, out_scale)[0], np.roll(z[0] * z[1], -step))


@pytest.mark.parametrize("public", [False, True], ids=["symmetric", "public"])
def test_ckks_round_trip_from_a_master_seed(public, gpu):
    import torch
    from phantom_fhe_amd import workloads as W
    name, level, scale, step = "hyb12_a2", 6, 2.0 ** 40, 1
    P, ctx = _ctx(name, gpu)
    log_n, primes, _ = _params(name)
    n, slots = 1 << log_n, 1 << (log_n - 1)
    enc, kind = ctx.ckks_encoder(), P.scheme_type.ckks
    elt = S.elt_of_step(step, n)
    keys = W.keygen(ctx, kind, galois_elts=(elt,), master=MASTER)
    z = S.messages(12, 2, slots)
    samples = W.sample_encryption(ctx, level, 2, MASTER, public=public)
    cts = W.encode_encrypt_batch(ctx, enc, torch.from_numpy(z).to(gpu), level, scale, keys["pk"] if public else keys["sk_ntt"], samples, public=public)
    if not public:
        assert cts.data_ptr() == samples[0].data_ptr()        # a was sampled where c1 lies: the buffer is the ciphertext batch
    t3, prod = _poisoned((3, level, n), gpu), _poisoned((1, 2, level - 1, n), gpu)
    ctx.tensor_prod_2x2_rns_poly(cts[0], cts[1], t3, level)
    ctx.keyswitch_rescale(level, t3[:2], t3[2], keys["relin"].public_keys_ptr, prod[0])
    rot, g1 = _poisoned((1, 2, level - 1, n), gpu), _poisoned((1, level - 1, n), gpu)
    ctx.apply_galois_for_keyswitch(prod, rot, g1, elt, level - 1, 1, True)
    ctx.keyswitch_inplace(level - 1, rot[0], g1[0], keys["galois"][elt].public_keys_ptr, kind)
    out_scale = scale * scale / float(primes[level - 1])
    got = W.decrypt_decode_batch(ctx, enc, rot, level - 1, out_scale, keys["sk_powers"]).cpu().numpy()[0]
    want = np.roll(z[0] * z[1], -step)
    gpu_err, cpu_err = S.max_err(got, want), _cpu_product_then_rotation(level, scale, step)
    print(f"ckks round trip public={public}: cpu_err {cpu_err:.3e} gpu_err {gpu_err:.3e} bound {S.bound(cpu_err):.3e}")
    assert cpu_err < S.CPU_CAP
    assert gpu_err <= S.bound(cpu_err)
    assert S.nearest_wrong(got, S.rotation_wrongs(z[0] * z[1], step) + S.product_wrongs(z[0], z[1])) > S.FAR
    del enc, ctx
    _release()


def _rows(m):
    return np.asarray(m).reshape(2, -1)


@pytest.mark.parametrize("public", [False, True], ids=["symmetric", "public"])
@pytest.mark.parametrize("scheme,name", [(O.BGV, "hyb12_a2"), (O.BFV, "bfv13_50")], ids=["bgv", "bfv"])
def test_bgv_bfv_round_trip_from_a_master_seed(scheme, name, public, gpu):
    import torch
    from phantom_fhe_amd import workloads as W
    P, ctx = _ctx(name, gpu, T)
    log_n, primes, size_p = _params(name)
    n, level, step = 1 << log_n, len(primes) - size_p, 3
    kind = P.scheme_type.bgv if scheme == O.BGV else P.scheme_type.bfv
    enc = P.BatchEncoder(ctx)
    elt = S.elt_of_step(step, n)
    keys = W.keygen(ctx, kind, galois_elts=(elt,), master=MASTER)
    m = rng_for(8900 + scheme).integers(0, T, (2, n)).astype(np.int64)
    samples = W.sample_encryption(ctx, level, 2, MASTER, public=public)
    cts = W.batch_encode_encrypt(ctx, enc, torch.from_numpy(m).to(gpu), level, keys["pk"] if public else keys["sk_ntt"], samples, kind, public=public)
    back = W.batch_decrypt_decode(ctx, enc, cts, level, keys["sk_powers"], kind).cpu().numpy()
    assert np.array_equal(back, m), "encrypt -> decrypt does not return the messages"
    ct3 = _poisoned((1, 3, level, n), gpu)
    if scheme == O.BGV:
        ctx.tensor_prod_2x2_rns_poly(cts[0], cts[1], ct3[0], level)
    else:
        ctx.bfv_multiply_behz(cts[0], cts[1], ct3[0])
    out = W.relinearize_rotate_batch(ctx, level, ct3, keys["relin"], keys["galois"][elt], elt, kind)
    got = W.batch_decrypt_decode(ctx, enc, out, level, keys["sk_powers"], kind).cpu().numpy()[0]
    prod = (_rows(m[0]) * _rows(m[1])) % T                       # below 2^34: exact in int64
    want = np.roll(prod, -step, axis=1).reshape(-1)
    assert not np.array_equal(prod.reshape(-1), want)
    assert np.array_equal(got, want), f"{int(np.count_nonzero(got != want))} of {n} slots differ from the rotated product"
    del enc, ctx
    _release()


def test_the_same_master_gives_the_same_words_and_another_master_other_keys(gpu):
    from phantom_fhe_amd import workloads as W
    name = "hyb12_a2"
    P, ctx = _ctx(name, gpu)
    kind = P.scheme_type.ckks

    def words(master):
        k = W.keygen(ctx, kind, galois_elts=(5,), master=master)
        ct, e = W.sample_encryption(ctx, 3, 2, master)
        u, e2 = W.sample_encryption(ctx, 3, 2, master, public=True)
        return [P.to_host(x) for x in [k["sk_ntt"], k["sk_powers"], k["pk"]] + k["relin"].public_keys + k["galois"][5].public_keys
                + [ct[:, 1].contiguous(), e, u, e2]]

    first, again, other = words(MASTER), words(MASTER), words(bytes(64))
    assert all(np.array_equal(x, y) for x, y in zip(first, again))
    assert not any(np.array_equal(x, y) for x, y in zip(first, other))
    fresh = W.keygen(ctx, kind)                                   # master=None: fresh entropy, returned with the keys
    assert len(fresh["master"]) == 64 and not np.array_equal(P.to_host(fresh["sk_ntt"]), first[0])
    del ctx
    _release()


# ------------------------------------------------------------------------------------------------------------------------------
# F: refusals, count == 0, graph capture
# ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_empty_batch(gpu):
    import torch
    from phantom_fhe_amd import lib as L
    name = "hyb12_a2"
    P, ctx = _ctx(name, gpu)
    log_n, primes, size_p = _params(name)
    n, size_qp, size_q = 1 << log_n, len(primes), len(primes) - size_p
    lib, h, st = ctx._L, ctx._h, torch.cuda.current_stream().cuda_stream
    seeds = _dseeds(np.stack([_seed_of(name, b) for b in range(12)]), gpu)
    out = _poisoned((2, 2 * size_qp * n + PAD), gpu)
    sk = P.to_device(np.ones((size_qp, n), dtype=np.uint64), gpu)
    nk = P.to_device(np.ones((2, size_q, n), dtype=np.uint64), gpu)
    o, s = out.data_ptr(), seeds.data_ptr()
    ckks = int(P.scheme_type.ckks)
    refused = [
        ("null out", lambda: lib.pha_sample_ternary_poly(h, None, s, 1, 0, st)),
        ("null seed", lambda: lib.pha_sample_uniform_poly(h, o, None, 1, 0, st)),
        ("rows outside the context", lambda: lib.pha_sample_error_poly(h, o, s, size_qp, 1, st)),
        ("no rows", lambda: lib.pha_sample_uniform_poly(h, o, s, 0, 0, st)),
        ("start outside the context", lambda: lib.pha_sample_ternary_poly(h, o, s, 1, size_qp + 1, st)),
        ("unaligned out", lambda: lib.pha_sample_uniform_poly(h, o + 8, s, 1, 0, st)),
        ("unaligned seed", lambda: lib.pha_sample_ternary_poly(h, o, s + 4, 1, 0, st)),
        ("count above the grid limit", lambda: lib.pha_sample_error_signed_batched(h, s, 65536, o, n, st)),
        ("odd stride", lambda: lib.pha_sample_ternary_signed_batched(h, s, 2, o, n + 1, st)),
        ("short stride", lambda: lib.pha_sample_error_signed_batched(h, s, 2, o, n - 2, st)),
        ("null seeds", lambda: lib.pha_sample_error_signed_batched(h, None, 1, o, n, st)),
        ("level 0", lambda: lib.pha_sample_uniform_batched(h, 0, 0, s, 1, o, n, st)),
        ("level above |Q|", lambda: lib.pha_sample_uniform_batched(h, size_q + 1, 0, s, 1, o, (size_q + 1) * n, st)),
        ("short uniform stride", lambda: lib.pha_sample_uniform_batched(h, 3, 1, s, 2, o, 3 * n, st)),
        ("odd uniform stride", lambda: lib.pha_sample_uniform_batched(h, 1, 0, s, 2, o, n + 1, st)),
        ("null sk", lambda: lib.pha_secret_key_generate(h, s, None, st)),
        ("null new keys", lambda: lib.pha_generate_kswitch_keys_seeded(h, sk.data_ptr(), None, 1, size_q * n, s, o, 2 * size_qp * n, ckks, st)),
        ("short evk stride", lambda: lib.pha_generate_kswitch_keys_seeded(h, sk.data_ptr(), nk.data_ptr(), 1, size_q * n, s, o, 2 * size_qp * n - 2, ckks, st)),
        ("short new-key stride", lambda: lib.pha_generate_kswitch_keys_seeded(h, sk.data_ptr(), nk.data_ptr(), 2, size_q * n - 2, s, o, 2 * size_qp * n, ckks, st)),
        ("unknown scheme", lambda: lib.pha_generate_kswitch_keys_seeded(h, sk.data_ptr(), nk.data_ptr(), 1, size_q * n, s, o, 2 * size_qp * n, 9, st)),
        ("bgv without a plain modulus", lambda: lib.pha_generate_kswitch_keys_seeded(h, sk.data_ptr(), nk.data_ptr(), 1, size_q * n, s, o, 2 * size_qp * n, int(P.scheme_type.bgv), st)),
        ("too many keys", lambda: lib.pha_generate_kswitch_keys_seeded(h, sk.data_ptr(), nk.data_ptr(), 65536, size_q * n, s, o, 2 * size_qp * n, ckks, st)),
        ("evk overlapping the key", lambda: lib.pha_generate_kswitch_keys_seeded(h, sk.data_ptr(), nk.data_ptr(), 1, size_q * n, s, sk.data_ptr(), 2 * size_qp * n, ckks, st)),
    ]
    for what, call in refused:
        assert call() == -1, what
        assert lib.pha_last_error(), what
    # count == 0 does nothing and succeeds
    assert lib.pha_sample_ternary_signed_batched(h, s, 0, o, n, st) == 0
    assert lib.pha_sample_error_signed_batched(h, s, 0, o, n, st) == 0
    assert lib.pha_sample_uniform_batched(h, 3, 1, s, 0, o, 0, st) == 0
    assert lib.pha_generate_kswitch_keys_seeded(h, sk.data_ptr(), nk.data_ptr(), 0, size_q * n, s, o, 2 * size_qp * n, ckks, st) == 0
    torch.cuda.synchronize()
    assert bool((out == POISON).all()), "a refused or empty call wrote to its output"
    # a context without special primes: with_special and key generation are refused
    P2, plain_ctx = _ctx("c2_ntt14", gpu)
    big = _poisoned((8 * (1 << 14),), gpu)
    assert plain_ctx._L.pha_sample_uniform_batched(plain_ctx._h, 2, 1, s, 1, big.data_ptr(), 0, st) == -1
    assert plain_ctx._L.pha_generate_kswitch_keys_seeded(plain_ctx._h, big.data_ptr(), big.data_ptr(), 1, 0, s, big.data_ptr(), 0, ckks, st) == -1
    assert bool((big == POISON).all())
    # the Python layer checks what it can see
    with pytest.raises(ValueError):
        ctx.sample_ternary_signed_batched(seeds[:1], _poisoned((2, n), gpu))       # two polynomials, one seed
    with pytest.raises(ValueError):
        ctx.sample_uniform_poly(out[0], seeds.to(torch.int64), 1)                   # seeds are uint8
    with pytest.raises(ValueError):
        L.check(-1)
    del ctx, plain_ctx
    _release()


def test_key_generation_captured_into_a_graph(gpu):
    import torch
    name = "hyb12_a2"
    P, ctx = _ctx(name, gpu)
    log_n, primes, size_p = _params(name)
    n, size_qp, size_q = 1 << log_n, len(primes), len(primes) - size_p
    dnum, n_keys, kind = size_q // size_p, 2, P.scheme_type.ckks
    rng = rng_for(8950)
    new_keys = P.to_device(np.stack([np.stack([rng.integers(0, q, n, dtype=np.uint64) for q in primes[:size_q]]) for _ in range(n_keys)]), gpu)
    host_seeds = [np.stack([_seed_of(name, 70 + 20 * r + i) for i in range(2 * n_keys * dnum)]) for r in range(2)]
    seeds = _dseeds(host_seeds[0], gpu)
    sk = ctx.secret_key_generate(_dseeds(_seed_of(name, 69), gpu))
    want = []
    for r in range(2):                                            # eager results for two sets of seeds
        evk = _poisoned((n_keys, dnum, 2, size_qp, n), gpu)
        ctx.generate_kswitch_keys_seeded(sk, new_keys, _dseeds(host_seeds[r], gpu), kind, evk=evk)
        want.append(P.to_host(evk))
    assert not np.array_equal(want[0], want[1])
    evk = _poisoned((n_keys, dnum, 2, size_qp, n), gpu)

    def call():
        st = torch.cuda.current_stream().cuda_stream
        assert ctx._L.pha_generate_kswitch_keys_seeded(ctx._h, sk.data_ptr(), new_keys.data_ptr(), n_keys, size_q * n, seeds.data_ptr(),
                                                       evk.data_ptr(), 2 * size_qp * n, int(kind), st) == 0

    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                                    # warm-up on the capture stream: the stream's arena exists before the capture
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            call()
    for r in (1, 0):
        seeds.copy_(_dseeds(host_seeds[r], gpu))
        evk.fill_(POISON)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(P.to_host(evk), want[r]), f"the replayed graph differs from the eager call (seeds {r})"
    del g, ctx
    _release()
