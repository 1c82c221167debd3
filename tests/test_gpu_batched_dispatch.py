"""GPU parity of the batched key switch where its dispatch changes, bit-exact against the CPU oracle, every output word of every
ciphertext compared:

A. more than four key-switch digits with alpha > 1 (hyb13_b5, hyb14_b6, hyb16_b5), stage by stage and whole, one ciphertext: the
   unfused mod-up + inner product (fusable_ip() is false), key switch + rescale, hoisting, weighted hoisting; the baby-step /
   giant-step form refuses beta > 4 and works at the beta = 4 level of the same context;
B. the same sets through the batched entries: the per-ciphertext inner product loop, the mod-up that COPIES the digits' own limbs
   (at N = 2^16 below and above the 1024-workgroup threshold of the fused conversion), one context crossing beta 5 -> 4 -> 5;
C. both sides of each workgroup threshold of the fused conversions at N = 2^16 (c3_ckks16 B = 6, 7, 9; hyb16_a12 B = 7, 8);
D. the batch sizes bench.py times (c3_ckks16, level 45, B = 16 and 32), also word for word against B single-ciphertext calls;
E. extreme residues (q - 1, 0, q - 1 - r) inside a batch (in B and C) and keys at q - 1 through the beta > 4 stages;
F. argument edges of the batched entries.

Which kernels each group launches is recorded in profiles/r07_batched_dispatch_kernels.md."""
import gc

import numpy as np
import pytest

from oracle import oracle as O
from util import BETA_GT4_LEVELS, oracle_ctx, primes_of, rng_for, uniform_poly

pytestmark = pytest.mark.gpu

BGV_T = 65537
SCHEMES = {"ckks": O.CKKS, "bfv": O.BFV, "bgv": O.BGV}
_DIMS = ("ciphertext", "polynomial", "limb", "index")


def _setup(name, scheme, gpu):
    import phantom_fhe_amd as P
    log_n, primes, size_p = primes_of(name)
    ctx = P.PhantomContext(log_n, list(primes), size_p, device=gpu)
    if scheme == O.BGV:
        ctx.set_plain_modulus(BGV_T)
    return P, oracle_ctx(name), ctx, log_n, primes, size_p, len(primes) - size_p


def _tool(oc, ql, scheme):
    tool = O.Tool(oc, ql)
    if scheme == O.BGV:
        tool.set_plain_modulus(BGV_T)
    return tool


def _release():
    import torch
    gc.collect()
    torch.cuda.empty_cache()


def _top(ps, n):
    return np.stack([np.full(n, int(q) - 1, dtype=np.uint64) for q in ps])


def _keys(rng, primes, n, dnum, top=False):
    """Synthetic evaluation keys [dnum][2][QP][N]: uniform, or q - 1 everywhere."""
    if top:
        return np.stack([np.stack([_top(primes, n)] * 2)] * dnum)
    return np.stack([np.stack([uniform_poly(rng, primes, n), uniform_poly(rng, primes, n)]) for _ in range(dnum)])


def _check(got, ref, what, ql, alpha, lead=(), dims=_DIMS):
    """Bit-exact comparison; on a mismatch names the first differing (ciphertext, polynomial, limb, index) and whether that limb is
    an own limb of some digit (every data limb j < ql is the own limb of digit j // alpha) or a special limb."""
    assert got.shape == ref.shape, f"{what}: shape {got.shape} != {ref.shape}"
    if np.array_equal(got, ref):
        return
    idx = tuple(int(v) for v in lead) + tuple(int(v) for v in np.argwhere(got != ref)[0])
    limb = idx[-2]
    where = f"own limb of digit {limb // alpha}" if limb < ql else f"special limb {limb - ql}"
    names = dims[len(dims) - len(idx):]
    at = ", ".join(f"{k} {v}" for k, v in zip(names, idx))
    sub = idx[len(lead):]
    msg = (f"{what}: {int(np.count_nonzero(got != ref))} words differ, first at {at} ({where}): "
           f"got {int(got[sub])}, want {int(ref[sub])}")
    print(msg)
    raise AssertionError(msg)


def _batch_inputs(rng, primes, ql, n, batch, extreme=False):
    """ct [B][2][Ql][N], c2 [B][Ql][N], uniform; extreme: ciphertext 0 at q - 1 in every limb, ciphertext B - 1 all zero, the middle
    one at q - 1 - r, r < 2^16 (residues just below q with busy low bits)."""
    ct = np.stack([np.stack([uniform_poly(rng, primes[:ql], n) for _ in range(2)]) for _ in range(batch)])
    c2 = np.stack([uniform_poly(rng, primes[:ql], n) for _ in range(batch)])
    if extreme:
        assert batch >= 3
        q = np.array([int(p) for p in primes[:ql]], dtype=np.uint64)[:, None]
        ct[0], c2[0] = q - 1, q - 1
        ct[batch - 1], c2[batch - 1] = 0, 0
        m = batch // 2
        ct[m] = q - 1 - rng.integers(0, 1 << 16, (2, ql, n), dtype=np.uint64)
        c2[m] = q - 1 - rng.integers(0, 1 << 16, (ql, n), dtype=np.uint64)
    return ct, c2


def _check_batched_keyswitch(P, ctx, tool, scheme, rlk, evk, ct, c2, ql, alpha, gpu, rescale=True):
    """keyswitch_rescale_batched (ckks) and keyswitch_inplace_batched on one batch: every ciphertext against the oracle's
    keyswitch_inplace (and rescale_ntt of it); the inputs the entries declare const come back unchanged.  Returns the device results
    (rescaled or None, key-switched) for further comparisons."""
    batch, n = ct.shape[0], ct.shape[-1]
    keys = [evk[i] for i in range(tool.beta)]
    ref = [tool.keyswitch_inplace(ct[b], c2[b], keys, scheme) for b in range(batch)]
    d_ct, d_c2 = P.to_device(ct, gpu), P.to_device(c2, gpu)
    dst = None
    tag = f"ql={ql} beta={tool.beta} B={batch}"
    if rescale and scheme == O.CKKS and ql > 1:
        dst = P.to_device(np.zeros((batch, 2, ql - 1, n), dtype=np.uint64), gpu)
        ctx.keyswitch_rescale_batched(ql, d_ct, d_c2, batch, rlk.public_keys_ptr, dst)
        got = P.to_host(dst)
        for b in range(batch):
            _check(got[b], tool.rescale_ntt(ref[b], 2), f"keyswitch_rescale_batched {tag}", ql, alpha, lead=(b,))
        assert np.array_equal(P.to_host(d_ct), ct), f"keyswitch_rescale_batched {tag} wrote to ct"
        assert np.array_equal(P.to_host(d_c2), c2), f"keyswitch_rescale_batched {tag} wrote to c2"
        del got
    ctx.keyswitch_inplace_batched(ql, d_ct, d_c2, batch, rlk.public_keys_ptr, scheme)
    got = P.to_host(d_ct)
    for b in range(batch):
        _check(got[b], ref[b], f"keyswitch_inplace_batched {tag}", ql, alpha, lead=(b,))
    assert np.array_equal(P.to_host(d_c2), c2), f"keyswitch_inplace_batched {tag} wrote to c2"
    return dst, d_ct


def _relin_rotate_reference(oc, tool, log_n, ct3, keys, gkeys, elt, scheme):
    """The oracle's three steps per ciphertext: relinearize, Galois permutation, key switch of the rotated c1."""
    n, ql = tool.n, tool.size_ql
    table = O.galois_ntt_table(log_n, elt)
    out = []
    for b in range(ct3.shape[0]):
        x = tool.keyswitch_inplace(ct3[b, :2], ct3[b, 2], keys, scheme)
        if scheme == O.BFV:
            g = [oc.apply_galois_coeff(x[p], elt, ql) for p in range(2)]
        else:
            g = [O.apply_galois_ntt(x[p], table, n, ql) for p in range(2)]
        out.append(tool.keyswitch_inplace(np.stack([g[0], np.zeros_like(g[0])]), g[1], gkeys, scheme))
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# A / E: beta > 4, one ciphertext, stage by stage and whole
# ------------------------------------------------------------------------------------------------------------------------------
def _run_stages(name, scheme, levels, gpu, extreme=False):
    P, oc, ctx, log_n, primes, size_p, size_q = _setup(name, scheme, gpu)
    n = 1 << log_n
    r = rng_for(8100 + log_n)
    dnum = -(-size_q // size_p)
    evk = _keys(r, primes, n, dnum, top=extreme)
    rlk = P.PhantomRelinKey.from_numpy(evk, gpu)
    elts = [5, 2 * n - 1]
    glk = [_keys(r, primes, n, dnum, top=extreme) for _ in elts]
    d_glk = [P.PhantomRelinKey.from_numpy(k, gpu) for k in glk]
    for ql in levels:
        tool = _tool(oc, ql, scheme)
        qlp, beta = ql + size_p, tool.beta
        assert beta == BETA_GT4_LEVELS[name][ql] and ctx.beta(ql) == beta
        keys = [evk[i] for i in range(beta)]
        tag = f"{name} ql={ql} beta={beta}"
        c2s = [_top(primes[:ql], n), np.zeros((ql, n), dtype=np.uint64)] if extreme else [uniform_poly(r, primes[:ql], n)]
        for c2 in c2s:
            # mod-up: beta > 4 copies the digits' own limbs into the digit buffers
            d_mu = P.to_device(np.zeros((beta, qlp, n), dtype=np.uint64), gpu)
            ctx.modup(ql, d_mu, P.to_device(c2, gpu), scheme)
            ref_mu = tool.modup(c2, scheme)
            _check(P.to_host(d_mu), ref_mu, f"modup {tag}", ql, size_p, dims=("digit", "limb", "index"))
            # inner product over beta > 4 digits
            d_cx = P.to_device(np.zeros((2, qlp, n), dtype=np.uint64), gpu)
            ctx.key_switch_inner_prod(ql, d_cx, d_mu, rlk.public_keys_ptr)
            ref_cx = tool.key_switch_inner_prod(ref_mu, keys)
            _check(P.to_host(d_cx), ref_cx, f"inner product {tag}", ql, size_p)
            for i in range(2):      # mod-down, in place like keyswitch_inplace does
                ctx.moddown_from_NTT(ql, d_cx[i], d_cx[i], scheme)
                _check(P.to_host(d_cx[i])[:ql], tool.moddown_from_ntt(ref_cx[i], scheme), f"moddown {tag} poly={i}", ql, size_p)
            # the whole key switch: fusable_ip() is false, so mod-up and inner product are separate launches
            if extreme:
                ct = np.stack([_top(primes[:ql], n)] * 2)
            else:
                ct = np.stack([uniform_poly(r, primes[:ql], n), uniform_poly(r, primes[:ql], n)])
            d_ct, d_c2 = P.to_device(ct, gpu), P.to_device(c2, gpu)
            ctx.keyswitch_inplace(ql, d_ct, d_c2, rlk.public_keys_ptr, scheme)
            ref_ks = tool.keyswitch_inplace(ct, c2, keys, scheme)
            _check(P.to_host(d_ct), ref_ks, f"keyswitch_inplace {tag}", ql, size_p)
            if scheme == O.CKKS and ql > 1:     # key switch + rescale in one call: the last-limb fix in the unfused inner product
                d_ct = P.to_device(ct, gpu)
                dst = P.to_device(np.zeros((2, ql - 1, n), dtype=np.uint64), gpu)
                ctx.keyswitch_rescale(ql, d_ct, d_c2, rlk.public_keys_ptr, dst)
                _check(P.to_host(dst), tool.rescale_ntt(ref_ks, 2), f"keyswitch_rescale {tag}", ql, size_p)
                assert np.array_equal(P.to_host(d_ct), ct) and np.array_equal(P.to_host(d_c2), c2), f"keyswitch_rescale {tag} wrote to its inputs"
        # hoisted rotations: one shared mod-up over beta digits, two Galois elements
        o_glk = [[k[i] for i in range(beta)] for k in glk]
        d_h = P.to_device(ct, gpu)
        ctx.hoisting(ql, d_h, elts, d_glk, scheme)
        _check(P.to_host(d_h), tool.hoisting(ct, elts, o_glk, scheme), f"hoisting {tag}", ql, size_p)
        if scheme != O.BFV:     # weighted sum of the identity and both rotations (NTT-form schemes only)
            qlp_primes = [primes[i] for i in list(range(ql)) + [size_q + j for j in range(size_p)]]
            ws = [_top(qlp_primes, n) if extreme else uniform_poly(r, qlp_primes, n) for _ in range(3)]
            d_w = P.to_device(ct, gpu)
            ctx.hoisting_weighted(ql, d_w, [1] + elts, [None] + d_glk, [P.to_device(w, gpu) for w in ws], scheme)
            _check(P.to_host(d_w), tool.hoisting_weighted(ct, [1] + elts, [None] + o_glk, ws, scheme), f"hoisting_weighted {tag}", ql, size_p)
    del ctx, rlk, d_glk
    _release()


@pytest.mark.parametrize("scheme", list(SCHEMES))
@pytest.mark.parametrize("name", list(BETA_GT4_LEVELS))
def test_beta_gt4_stages(name, scheme, gpu):
    """modup, key_switch_inner_prod, moddown_from_NTT, keyswitch_inplace, keyswitch_rescale (ckks), hoisting with two Galois
    elements and hoisting_weighted at every listed level of the beta > 4 sets, all three schemes."""
    _run_stages(name, SCHEMES[scheme], list(BETA_GT4_LEVELS[name]), gpu)


@pytest.mark.parametrize("name,scheme,levels", [("hyb13_b5", "ckks", [10, 9]), ("hyb13_b5", "bfv", [10]), ("hyb13_b5", "bgv", [9]),
                                                ("hyb14_b6", "ckks", [12])])
def test_beta_gt4_stages_extreme_keys(name, scheme, levels, gpu):
    """The same stages with keys, ciphertext and weights at q - 1 throughout and c2 at q - 1, then 0: the largest sums the 128-bit
    inner product over five / six digits can hold."""
    _run_stages(name, SCHEMES[scheme], levels, gpu, extreme=True)


@pytest.mark.parametrize("scheme", ["ckks", "bgv"])
@pytest.mark.parametrize("name,ql_bad,ql_ok", [("hyb13_b5", 10, 8), ("hyb14_b6", 12, 8), ("hyb16_b5", 45, 36)])
def test_bsgs_refuses_beta_gt4_and_runs_at_beta4(name, ql_bad, ql_ok, scheme, gpu):
    """The baby-step / giant-step matrix-vector form raises ValueError with more than four digits (before any launch: the input is
    unchanged) and gives the oracle's composition at the beta = 4 level of the same context."""
    from phantom_fhe_amd import workloads as W
    scheme = SCHEMES[scheme]
    P, oc, ctx, log_n, primes, size_p, size_q = _setup(name, scheme, gpu)
    n = 1 << log_n
    r = rng_for(8200 + log_n)
    dnum = -(-size_q // size_p)
    elts = [5, 2 * n - 1]
    glk = [_keys(r, primes, n, dnum) for _ in elts]
    d_glk = [P.PhantomRelinKey.from_numpy(k, gpu) for k in glk]
    for ql in (ql_bad, ql_ok):
        tool = _tool(oc, ql, scheme)
        assert tool.beta == BETA_GT4_LEVELS[name][ql] and ctx.beta(ql) == tool.beta
        qlp_primes = [primes[i] for i in list(range(ql)) + [size_q + j for j in range(size_p)]]
        ct = np.stack([uniform_poly(r, primes[:ql], n) for _ in range(2)])
        ws = [[uniform_poly(r, qlp_primes, n) for _ in range(2)] for _ in range(2)]
        d_ws = [[P.to_device(w, gpu) for w in row] for row in ws]
        d_ct = P.to_device(ct, gpu)
        args = (ctx, ql, d_ct, [1, elts[0]], [None, d_glk[0]], [1, elts[1]], [None, d_glk[1]], d_ws, scheme)
        if ql == ql_bad:
            assert tool.beta > 4
            with pytest.raises(ValueError):
                W.diag_matvec_bsgs(*args)
            with pytest.raises(ValueError):
                ctx.hoisting_weighted_bsgs(ql, d_ct, *args[3:])         # in place: refused before anything is written
            assert np.array_equal(P.to_host(d_ct), ct)
        else:
            assert tool.beta == 4
            o_glk = [[k[i] for i in range(4)] for k in glk]
            ref = tool.hoisting_weighted_bsgs(ct, [1, elts[0]], [None, o_glk[0]], [1, elts[1]], [None, o_glk[1]], ws, scheme)
            _check(P.to_host(W.diag_matvec_bsgs(*args)), ref, f"diag_matvec_bsgs {name} ql={ql}", ql, size_p)
    del ctx, d_glk, d_ws
    _release()


# ------------------------------------------------------------------------------------------------------------------------------
# B / E: beta > 4 through the batched entries; one context and one scratch arena across beta 5 -> 4 -> 5
# ------------------------------------------------------------------------------------------------------------------------------
# (config, [(live data limbs, batch, extreme residues)]).  hyb16_b5: 3 x 5 = 15 digit polynomials stay below the 1024 workgroups
# of the fused conversion (bconv_kernel copies the own limbs), 4 x 5 = 20 are above (modup_conv_s1_kernel copies them); in between,
# level 36 (beta 4) takes the own-limbs-in-place path with the batched inner product; 37 has a one-limb last digit
B_STEPS = {
    "hyb13_b5": [(10, 2, False), (8, 3, False), (10, 3, True), (9, 2, False), (1, 2, False)],
    "hyb14_b6": [(12, 2, False), (8, 3, False), (12, 3, True)],
    "hyb16_b5": [(45, 3, False), (36, 4, False), (45, 4, True), (37, 4, False)],
}


@pytest.mark.parametrize("scheme", list(SCHEMES))
@pytest.mark.parametrize("name", list(B_STEPS))
def test_beta_gt4_batched(name, scheme, gpu):
    """keyswitch_inplace_batched (all schemes) and keyswitch_rescale_batched (ckks) with more than four digits: the inner product runs
    once per ciphertext on advancing pointers and the mod-up copies the own limbs; every ciphertext against the oracle, const inputs
    unchanged, and the beta = 4 level in between switches the same context to own-limbs-in-place and back."""
    scheme = SCHEMES[scheme]
    P, oc, ctx, log_n, primes, size_p, size_q = _setup(name, scheme, gpu)
    n = 1 << log_n
    r = rng_for(8300 + log_n)
    evk = _keys(r, primes, n, -(-size_q // size_p))
    rlk = P.PhantomRelinKey.from_numpy(evk, gpu)
    betas = []
    for ql, batch, extreme in B_STEPS[name]:
        if name == "hyb16_b5" and ql == 37 and scheme != O.CKKS:
            continue            # (the one-limb last digit at N = 2^16 once, under the scheme with both entries)
        tool = _tool(oc, ql, scheme)
        assert tool.beta == BETA_GT4_LEVELS[name][ql] and ctx.beta(ql) == tool.beta
        betas.append(tool.beta)
        ct, c2 = _batch_inputs(r, primes, ql, n, batch, extreme)
        _check_batched_keyswitch(P, ctx, tool, scheme, rlk, evk, ct, c2, ql, size_p, gpu)
    assert [b > 4 for b in betas[:3]] == [True, False, True]
    del ctx, rlk
    _release()


@pytest.mark.parametrize("name,scheme,ql,batch", [("hyb13_b5", "ckks", 10, 3), ("hyb13_b5", "bgv", 10, 3),
                                                  ("hyb16_b5", "ckks", 45, 4), ("hyb16_b5", "bgv", 45, 4)])
def test_beta_gt4_relinearize_rotate(name, scheme, ql, batch, gpu):
    """relinearize_rotate_batch with more than four digits against the oracle's three steps: with all ciphertexts in one set (both
    batched key switches take the per-ciphertext inner product) and with the library's own set size."""
    from phantom_fhe_amd import workloads as W
    scheme = SCHEMES[scheme]
    P, oc, ctx, log_n, primes, size_p, size_q = _setup(name, scheme, gpu)
    n = 1 << log_n
    r = rng_for(8400 + log_n)
    dnum = -(-size_q // size_p)
    evk, gk = _keys(r, primes, n, dnum), _keys(r, primes, n, dnum)
    rlk, d_gk = P.PhantomRelinKey.from_numpy(evk, gpu), P.PhantomRelinKey.from_numpy(gk, gpu)
    tool = _tool(oc, ql, scheme)
    assert tool.beta > 4
    elt = 5
    ct3 = np.stack([np.stack([uniform_poly(r, primes[:ql], n) for _ in range(3)]) for _ in range(batch)])
    ref = _relin_rotate_reference(oc, tool, log_n, ct3, [evk[i] for i in range(tool.beta)], [gk[i] for i in range(tool.beta)], elt, scheme)
    d3 = P.to_device(ct3, gpu)
    for chunk in (batch, 0):
        got = P.to_host(W.relinearize_rotate_batch(ctx, ql, d3, rlk, d_gk, elt, scheme, chunk=chunk))
        for b in range(batch):
            _check(got[b], ref[b], f"relinearize_rotate_batch {name} ql={ql} B={batch} chunk={chunk}", ql, size_p, lead=(b,))
        assert np.array_equal(P.to_host(d3), ct3), "relinearize_rotate_batch wrote to ct3"
    del ctx, rlk, d_gk, d3
    _release()


# ------------------------------------------------------------------------------------------------------------------------------
# C / E: both sides of the 1024-workgroup thresholds at N = 2^16 in the product library
# ------------------------------------------------------------------------------------------------------------------------------
# c3_ckks16 (beta 3): the mod-up conversion is fused from beta * B >= 16 (B >= 6), the mod-down / rescale conversions from 2 B >= 16:
# B = 6 and 7 run the fused mod-up next to the SEPARATE mod-down / rescale conversion, B = 9 all three fused (B = 5 and 8 are in
# tests/test_gpu_rns.py).  Level 31 has a one-limb last digit.  B = 7 at the top level carries the extreme ciphertexts.
@pytest.mark.parametrize("ql,batch,extreme", [(45, 6, False), (45, 7, True), (45, 9, False), (31, 6, False), (31, 7, False)])
def test_threshold_sides_c3(ql, batch, extreme, gpu):
    name, scheme = "c3_ckks16", O.CKKS
    P, oc, ctx, log_n, primes, size_p, size_q = _setup(name, scheme, gpu)
    n = 1 << log_n
    r = rng_for(8500 + ql + batch)
    evk = _keys(r, primes, n, size_q // size_p)
    rlk = P.PhantomRelinKey.from_numpy(evk, gpu)
    tool = _tool(oc, ql, scheme)
    assert tool.beta == 3
    ct, c2 = _batch_inputs(r, primes, ql, n, batch, extreme)
    _check_batched_keyswitch(P, ctx, tool, scheme, rlk, evk, ct, c2, ql, size_p, gpu)
    del ctx, rlk
    _release()


# hyb16_a12 (beta 2): the fused mod-up needs B >= 8 -- the first time the product library reaches it under BGV
@pytest.mark.parametrize("scheme,batch", [("ckks", 7), ("ckks", 8), ("bgv", 8)])
def test_threshold_sides_a12(scheme, batch, gpu):
    name, ql = "hyb16_a12", 24
    scheme = SCHEMES[scheme]
    P, oc, ctx, log_n, primes, size_p, size_q = _setup(name, scheme, gpu)
    n = 1 << log_n
    r = rng_for(8600 + batch)
    evk = _keys(r, primes, n, size_q // size_p)
    rlk = P.PhantomRelinKey.from_numpy(evk, gpu)
    tool = _tool(oc, ql, scheme)
    assert tool.beta == 2
    ct, c2 = _batch_inputs(r, primes, ql, n, batch)
    _check_batched_keyswitch(P, ctx, tool, scheme, rlk, evk, ct, c2, ql, size_p, gpu)
    del ctx, rlk
    _release()


# relinearize + rotate in an NTT-form scheme at N = 2^16: sets of 8 (2 x 8 = 16 digit polynomials: the fused mod-up), the library's
# own set size for 8 ciphertexts (5 + 3, one stream), and 10 ciphertexts with chunk = 0: sets of 2 alternating over the two
# internal streams (two lanes need batch >= 2 x the 5 ciphertexts that fit the set budget at this size)
@pytest.mark.parametrize("batch,chunk", [(8, 8), (8, 0), (10, 0)])
def test_relinearize_rotate_a12_sets(batch, chunk, gpu):
    from phantom_fhe_amd import workloads as W
    name, ql, scheme, elt = "hyb16_a12", 24, O.CKKS, 5
    P, oc, ctx, log_n, primes, size_p, size_q = _setup(name, scheme, gpu)
    n = 1 << log_n
    r = rng_for(8700 + batch)
    dnum = size_q // size_p
    evk, gk = _keys(r, primes, n, dnum), _keys(r, primes, n, dnum)
    rlk, d_gk = P.PhantomRelinKey.from_numpy(evk, gpu), P.PhantomRelinKey.from_numpy(gk, gpu)
    tool = _tool(oc, ql, scheme)
    ct3 = np.stack([np.stack([uniform_poly(r, primes[:ql], n) for _ in range(3)]) for _ in range(batch)])
    ref = _relin_rotate_reference(oc, tool, log_n, ct3, [evk[i] for i in range(tool.beta)], [gk[i] for i in range(tool.beta)], elt, scheme)
    d3 = P.to_device(ct3, gpu)
    got = P.to_host(W.relinearize_rotate_batch(ctx, ql, d3, rlk, d_gk, elt, scheme, chunk=chunk))
    for b in range(batch):
        _check(got[b], ref[b], f"relinearize_rotate_batch {name} B={batch} chunk={chunk}", ql, size_p, lead=(b,))
    assert np.array_equal(P.to_host(d3), ct3), "relinearize_rotate_batch wrote to ct3"
    del ctx, rlk, d_gk, d3
    _release()


# a last set of ONE ciphertext (3 = 2 + 1): both of its key switches take what the single entry takes at N = 2^14, the fused mod-up +
# inner product -- under ckks with the folded inverse pass (the first one stores, the second accumulates), under bfv from
# coefficient-form input; c2 of the first one is read where it lies in ct3
@pytest.mark.parametrize("name,scheme", [("hyb14_a4", "ckks"), ("hyb14_a2", "bfv")])
def test_relinearize_rotate_last_set_of_one(name, scheme, gpu):
    from phantom_fhe_amd import workloads as W
    scheme, ql, batch, elt = SCHEMES[scheme], 8, 3, 5
    P, oc, ctx, log_n, primes, size_p, size_q = _setup(name, scheme, gpu)
    n = 1 << log_n
    r = rng_for(8800 + size_p)
    dnum = size_q // size_p
    evk, gk = _keys(r, primes, n, dnum), _keys(r, primes, n, dnum)
    rlk, d_gk = P.PhantomRelinKey.from_numpy(evk, gpu), P.PhantomRelinKey.from_numpy(gk, gpu)
    tool = _tool(oc, ql, scheme)
    assert tool.beta == dnum <= 4
    ct3 = np.stack([np.stack([uniform_poly(r, primes[:ql], n) for _ in range(3)]) for _ in range(batch)])
    ref = _relin_rotate_reference(oc, tool, log_n, ct3, [evk[i] for i in range(tool.beta)], [gk[i] for i in range(tool.beta)], elt, scheme)
    d3 = P.to_device(ct3, gpu)
    got = P.to_host(W.relinearize_rotate_batch(ctx, ql, d3, rlk, d_gk, elt, scheme, chunk=2))
    for b in range(batch):
        _check(got[b], ref[b], f"relinearize_rotate_batch {name} B={batch} chunk=2", ql, size_p, lead=(b,))
    whole = P.to_host(W.relinearize_rotate_batch(ctx, ql, d3, rlk, d_gk, elt, scheme, chunk=batch))
    _check(got, whole, f"relinearize_rotate_batch {name} B={batch} chunk=2 vs chunk={batch}", ql, size_p)
    assert np.array_equal(P.to_host(d3), ct3), "relinearize_rotate_batch wrote to ct3"
    del ctx, rlk, d_gk, d3
    _release()


# ------------------------------------------------------------------------------------------------------------------------------
# D: the shapes bench.py times
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [16, 32])
def test_timed_shapes_c3(batch, gpu):
    """c3_ckks16, 45 limbs, B = 16 and 32: tensor_prod_2x2_batched then keyswitch_rescale_batched (the batched HomMul of bench.py) and
    keyswitch_inplace_batched.  Every ciphertext against the oracle (one oracle key switch serves both entries: the rescale form is
    rescale_ntt of it), and the whole batch word for word against B single-ciphertext calls, which run the fused mod-up + inner
    product -- a different set of kernels."""
    import torch
    name, scheme = "c3_ckks16", O.CKKS
    P, oc, ctx, log_n, primes, size_p, size_q = _setup(name, scheme, gpu)
    n, ql = 1 << log_n, size_q
    r = rng_for(8800 + batch)
    evk = _keys(r, primes, n, size_q // size_p)
    rlk = P.PhantomRelinKey.from_numpy(evk, gpu)
    tool = _tool(oc, ql, scheme)
    keys = [evk[i] for i in range(tool.beta)]
    ct1, _ = _batch_inputs(r, primes, ql, n, batch)
    ct2 = np.stack([np.stack([uniform_poly(r, primes[:ql], n) for _ in range(2)]) for _ in range(batch)])
    d01 = P.to_device(ct1, gpu)
    d2 = P.to_device(np.zeros((batch, ql, n), dtype=np.uint64), gpu)
    d_ct2 = P.to_device(ct2, gpu)
    ctx.tensor_prod_2x2_batched(d01, d_ct2, d01, d2, ql, batch)         # in place on operand 1, as the bench calls it
    del d_ct2
    keep01, keep2 = d01.clone(), d2.clone()
    dst = P.to_device(np.zeros((batch, 2, ql - 1, n), dtype=np.uint64), gpu)
    ctx.keyswitch_rescale_batched(ql, d01, d2, batch, rlk.public_keys_ptr, dst)
    assert torch.equal(d01, keep01) and torch.equal(d2, keep2), "keyswitch_rescale_batched wrote to its inputs"
    d_ks = d01.clone()
    ctx.keyswitch_inplace_batched(ql, d_ks, d2, batch, rlk.public_keys_ptr, scheme)
    assert torch.equal(d2, keep2), "keyswitch_inplace_batched wrote to c2"
    del keep01, keep2
    for b in range(batch):      # (one ciphertext at a time: the host never holds more than the inputs)
        ref3 = oc.tensor_prod_2x2(ct1[b], ct2[b], ql)
        _check(P.to_host(d01[b]), ref3[:2], f"tensor_prod_2x2_batched B={batch} (c0, c1)", ql, size_p, lead=(b,))
        _check(P.to_host(d2[b]), ref3[2], f"tensor_prod_2x2_batched B={batch} c2", ql, size_p, lead=(b,), dims=("ciphertext", "limb", "index"))
        ref = tool.keyswitch_inplace(ref3[:2], ref3[2], keys, scheme)
        _check(P.to_host(d_ks[b]), ref, f"keyswitch_inplace_batched B={batch}", ql, size_p, lead=(b,))
        _check(P.to_host(dst[b]), tool.rescale_ntt(ref, 2), f"keyswitch_rescale_batched B={batch}", ql, size_p, lead=(b,))
    del ct1, ct2
    # B separate calls: keyswitch_rescale reads d01, keyswitch_inplace then completes d01 in place
    one = torch.zeros_like(dst)
    for b in range(batch):
        ctx.keyswitch_rescale(ql, d01[b], d2[b], rlk.public_keys_ptr, one[b])
    if not torch.equal(dst, one):
        _check(P.to_host(dst), P.to_host(one), f"keyswitch_rescale_batched B={batch} vs {batch} keyswitch_rescale calls", ql, size_p)
    for b in range(batch):
        ctx.keyswitch_inplace(ql, d01[b], d2[b], rlk.public_keys_ptr, scheme)
    if not torch.equal(d_ks, d01):
        _check(P.to_host(d_ks), P.to_host(d01), f"keyswitch_inplace_batched B={batch} vs {batch} keyswitch_inplace calls", ql, size_p)
    del ctx, rlk, d01, d2, dst, d_ks, one
    _release()


# ------------------------------------------------------------------------------------------------------------------------------
# F: argument edges of the batched entries
# ------------------------------------------------------------------------------------------------------------------------------
def test_batched_argument_edges(gpu):
    """batch 0 returns without touching a poisoned output; batch 1025 is refused before any launch (the buffers really hold 1025
    ciphertexts of the smallest chain, so nothing could be read out of bounds if that check were ever lost); key switch + rescale
    needs a modulus to drop."""
    import torch
    name, ql = "c1_bfv4096", 2
    P, oc, ctx, log_n, primes, size_p, size_q = _setup(name, O.CKKS, gpu)
    n = 1 << log_n
    r = rng_for(8900)
    evk = _keys(r, primes, n, size_q // size_p)
    rlk = P.PhantomRelinKey.from_numpy(evk, gpu)
    big = 1025
    ct1, c21 = _batch_inputs(r, primes, ql, n, 1)
    d_ct = P.to_device(np.broadcast_to(ct1, (big, 2, ql, n)), gpu)
    d_c2 = P.to_device(np.broadcast_to(c21, (big, ql, n)), gpu)
    poison = -0x2152411021524111          # 0xDEADBEEFDEADBEEF as int64
    dst = torch.full((big, 2, ql - 1, n), poison, dtype=torch.int64, device=gpu)
    d3 = torch.cat([d_ct[:4], d_c2[:4, None]], dim=1).contiguous()
    out = torch.full((4, 2, ql, n), poison, dtype=torch.int64, device=gpu)
    keep_ct, keep_c2 = d_ct.clone(), d_c2.clone()
    # empty batch: nothing happens
    ctx.keyswitch_rescale_batched(ql, d_ct, d_c2, 0, rlk.public_keys_ptr, dst)
    ctx.relinearize_rotate_batched(ql, d3, 0, rlk.public_keys_ptr, rlk.public_keys_ptr, 5, O.CKKS, out)
    poisoned = torch.full_like(d_ct, poison)
    for scheme in SCHEMES.values():
        ctx.keyswitch_inplace_batched(ql, poisoned, d_c2, 0, rlk.public_keys_ptr, scheme)
    torch.cuda.synchronize()
    assert bool((dst == poison).all()) and bool((out == poison).all()) and bool((poisoned == poison).all())
    # one ciphertext too many
    for scheme in SCHEMES.values():
        with pytest.raises(ValueError):
            ctx.keyswitch_inplace_batched(ql, d_ct, d_c2, big, rlk.public_keys_ptr, scheme)
    with pytest.raises(ValueError):
        ctx.keyswitch_rescale_batched(ql, d_ct, d_c2, big, rlk.public_keys_ptr, dst)
    # the last remaining modulus cannot be dropped (buffers sized for the larger level)
    with pytest.raises(ValueError):
        ctx.keyswitch_rescale_batched(1, d_ct, d_c2, 2, rlk.public_keys_ptr, dst)
    with pytest.raises(ValueError):
        ctx.keyswitch_rescale(1, d_ct[0], d_c2[0], rlk.public_keys_ptr, dst[0])
    torch.cuda.synchronize()
    assert bool((dst == poison).all()) and torch.equal(d_ct, keep_ct) and torch.equal(d_c2, keep_c2)
    del ctx, rlk, d_ct, d_c2, dst, poisoned, keep_ct, keep_c2
    _release()
