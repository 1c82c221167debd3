"""The kernels on the sets of tests/modulus_shapes.py, word for word against the CPU oracle that tests/test_modulus_shapes.py pins by
definitions: primes at the bottom of a bit width (the far side of the 2^41 / 2^42 / 2^46 / 2^47 / 2^49 / 2^50 switches of
make_fpmod and build_prime_tables), limbs of 16 .. 30 bits, plain moduli from 2 to 59 bits -- moduli that coeff_modulus_create never
draws.  Messages are checked by the helper's Python-integer decryption, never by the library's own.

Outputs are poisoned before a call, operands compared with their upload after it, a failure names the limb and its bit length
(util.first_diff_limb).

A. context tables (pha_context_prime_info, pha_context_download_twiddle) on every set;
B. NTT: single and batched launchers (B = 1, 3), inverse with scale, the include-special-mod pair, round trips;
C. dyadic rows and the two sum kernels at every term count 1 .. 40 and at 143 and 203;
D. conversions and the key switch (plain, fused with the rescale, fused with the BGV modulus switch) at every level of edge12 and the levels of the other sets the digit structure changes at;
E. BGV: modulus switch, fused key switch + modulus switch, decryption and noise budget at every plain modulus;
F. BFV: every in-domain cell of modulus_shapes.BFV_CELLS through its single and batched multiply, the message of the GPU product,
   the leveled entries one level down, decryption and noise budget of the fresh operands;
G. refusals: no HPS base at bottom50 and tiny12, and the context goes on to multiply by BEHZ."""
import gc

import numpy as np
import pytest

import modulus_shapes as M
from bv_semantics import MIN_MARGIN
from oracle import oracle as O
from util import first_diff_limb, uniform_poly

pytestmark = pytest.mark.gpu

POISON = -0x2152411021524111
ALL_SETS = list(M.SETS)
NTT_SETS = ["edge12", "edge14", "small12", "tiny12", "pair12"]
ROW_SETS = ["edge12", "small12", "tiny12", "pair12"]
TERMS = list(range(1, 41)) + [143, 203]          # 143 and 203: the longest FP64 flush periods (44- and 45-bit limbs)
BGV_T = 40961                                    # below every limb of every set: the plain modulus of the fused BGV switch in D
KS_LEVELS = [("edge12", [8, 7, 6, 5, 4, 3, 2, 1]), ("edge14", [8, 7, 2]), ("small12", [6, 3]), ("tiny12", [4, 3])]


def _setup(name, gpu, plain_t=None):
    import phantom_fhe_amd as P
    log_n, qp, size_p = M.primes_of(name)
    ctx = P.PhantomContext(log_n, list(qp), size_p, device=gpu)
    if plain_t:
        ctx.set_plain_modulus(plain_t)
    return P, M.oracle_ctx(name), ctx, 1 << log_n, [int(q) for q in qp], size_p, len(qp) - size_p


def _release():
    import torch
    gc.collect()
    torch.cuda.empty_cache()


def _poisoned(shape, gpu, dtype=None):
    import torch
    return torch.full(shape, POISON if dtype is None else -0x21524111, dtype=dtype or torch.int64, device=gpu)


def _rng(name, *tag):
    return np.random.default_rng(M.seed_of(name, "gpu", *tag))


def _keys(rng, primes, n, size_q, size_p):
    """Synthetic evaluation keys [dnum][2][QP][N], uniform residues."""
    return np.stack([np.stack([uniform_poly(rng, primes, n), uniform_poly(rng, primes, n)]) for _ in range(-(-size_q // size_p))])


def _cts(rng, primes, n, count, polys=2):
    """[count][polys][L][N]: the first ciphertext has every word at q - 1, the rest are uniform."""
    out = np.stack([np.stack([uniform_poly(rng, primes, n) for _ in range(polys)]) for _ in range(count)])
    out[0] = np.array(primes, dtype=np.uint64)[None, :, None] - np.uint64(1)
    return out


# ---- A ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL_SETS)
def test_a_context_tables(name, gpu):
    P, oc, ctx, n, qp, size_p, size_q = _setup(name, gpu)
    for i, q in enumerate(qp):
        info = ctx.prime_info(i)
        assert info["value"] == q and info["const_ratio"] == O.const_ratio(q), (name, q)
        assert info["root"] == O.minimal_primitive_root(2 * n, q) and info["n_inv"] == oc.n_inv(i), (name, q)
        for which in range(4):
            assert np.array_equal(ctx.twiddle_row(i, which), oc.twiddle(i, which)), (name, q, q.bit_length(), which)
    del ctx
    _release()


# ---- B ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NTT_SETS)
def test_b_ntt_launchers(name, gpu):
    P, oc, ctx, n, qp, size_p, size_q = _setup(name, gpu)
    L = len(qp)
    rows = list(range(L))
    x = M.edge_inputs(_rng(name, "ntt"), qp, n)                     # [3][L][N]: uniform, all q - 1, q - 1 - small
    fwd = np.stack([oc.nwt_forward_map(v, rows) for v in x])
    inv = np.stack([oc.nwt_backward_map(v, rows) for v in x])
    # the single launchers over the data limbs, then over the special limbs (start index), every input
    for kind in range(3):
        for start, count in ((0, size_q), (size_q, size_p)):
            if not count:
                continue
            sl = slice(start, start + count)
            d = P.to_device(x[kind], gpu)
            ctx.nwt_2d_radix8_forward_inplace(d, count, start)
            want = x[kind].copy()
            want[sl] = fwd[kind, sl]
            first_diff_limb(P.to_host(d), want, f"{name} forward input {kind} limbs [{start}, {start + count})", qp)
            ctx.nwt_2d_radix8_backward_inplace(d, count, start)
            first_diff_limb(P.to_host(d), x[kind], f"{name} round trip input {kind}", qp)
            ctx.nwt_2d_radix8_backward_inplace(d, count, start)
            want[sl] = inv[kind, sl]
            first_diff_limb(P.to_host(d), want, f"{name} inverse input {kind} limbs [{start}, {start + count})", qp)
    # the batched launchers, B = 1 and 3, over the data limbs of [B][L + 1][N] (a poisoned guard limb between the polynomials)
    for batch in (1, 3):
        buf = np.full((batch, L + 1, n), 0xA5A5A5A5DEADBEEF, dtype=np.uint64)
        buf[:, :L] = x[:batch]
        for which, ref in (("forward", fwd), ("backward", inv)):
            d = P.to_device(buf, gpu)
            getattr(ctx, f"nwt_2d_radix8_{which}_inplace_batched")(d, size_q, 0, batch, (L + 1) * n)
            want = buf.copy()
            want[:, :size_q] = ref[:batch, :size_q]
            for z in range(batch):
                first_diff_limb(P.to_host(d)[z, :L], want[z, :L], f"{name} batched {which} B={batch} polynomial {z}", qp)
            assert np.array_equal(P.to_host(d)[:, L], buf[:, L]), "the guard limb was written to"
    # inverse with scale: out of place (source untouched) and in place
    r = _rng(name, "scale")
    s = np.array([(1, q - 1, 3, int(r.integers(1, q)))[i % 4] for i, q in enumerate(qp[:size_q])], dtype=np.uint64)
    sh = np.array([O.compute_shoup(int(v), int(q)) for v, q in zip(s, qp)], dtype=np.uint64)
    d_s, d_sh = P.to_device(s, gpu), P.to_device(sh, gpu)
    for kind in range(3):
        src = np.ascontiguousarray(x[kind, :size_q])
        scaled = oc.multiply_scalar(inv[kind, :size_q], s, size_q, 0)
        d_in, d_out = P.to_device(src, gpu), _poisoned((size_q, n), gpu)
        ctx.nwt_2d_radix8_backward_scale(d_out, d_in, size_q, 0, d_s, d_sh)
        first_diff_limb(P.to_host(d_out), scaled, f"{name} inverse with scale input {kind}", qp)
        assert np.array_equal(P.to_host(d_in), src)
        ctx.nwt_2d_radix8_backward_inplace_scale(d_in, size_q, 0, d_s, d_sh)
        first_diff_limb(P.to_host(d_in), scaled, f"{name} inverse with scale in place input {kind}", qp)
    # the include-special-mod pair on [Ql || P] one level down (the special rows are not adjacent to the data rows)
    if size_p:
        ql = size_q - 1
        idx = list(range(ql)) + list(range(size_q, L))
        ip = [qp[i] for i in idx]
        for kind in range(3):
            y = np.ascontiguousarray(x[kind][idx])
            d = P.to_device(y, gpu)
            ctx.nwt_2d_radix8_forward_inplace_include_special_mod(d, ql + size_p, 0, L, size_p)
            first_diff_limb(P.to_host(d), oc.nwt_forward_map(y, idx), f"{name} forward include_special_mod input {kind}", ip)
            ctx.nwt_2d_radix8_backward_inplace_include_special_mod(d, ql + size_p, 0, L, size_p)
            first_diff_limb(P.to_host(d), y, f"{name} include_special_mod round trip input {kind}", ip)
            ctx.nwt_2d_radix8_backward_inplace_include_special_mod(d, ql + size_p, 0, L, size_p)
            first_diff_limb(P.to_host(d), oc.nwt_backward_map(y, idx), f"{name} inverse include_special_mod input {kind}", ip)
    del ctx
    _release()


# ---- C ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ROW_SETS)
def test_c_dyadic_rows(name, gpu):
    P, oc, ctx, n, qp, size_p, size_q = _setup(name, gpu)
    L = size_q
    pl = qp[:L]
    x = M.edge_inputs(_rng(name, "rows"), pl, n)
    top = x[1]
    cases = [(x[0], x[2], x[1]), (top, top, top), (x[2], top, x[0])]
    for i, (a, b, d) in enumerate(cases):
        da, db, dd = (P.to_device(v, gpu) for v in (a, b, d))
        out = _poisoned((L, n), gpu)
        ctx.multiply_rns_poly(da, db, out, L)
        first_diff_limb(P.to_host(out), oc.multiply(a, b, L), f"{name} multiply case {i}", pl)
        out = _poisoned((L, n), gpu)
        ctx.multiply_and_add_rns_poly(da, db, dd, out, L)
        first_diff_limb(P.to_host(out), oc.multiply_and_add(a, b, d, L), f"{name} multiply_and_add case {i}", pl)
        ct1, ct2 = np.stack([a, b]), np.stack([d, a])
        buf = P.to_device(np.concatenate([ct1, np.zeros((1, L, n), dtype=np.uint64)]), gpu)
        ctx.tensor_prod_2x2_rns_poly(buf, P.to_device(ct2, gpu), buf, L)
        first_diff_limb(P.to_host(buf), oc.tensor_prod_2x2(ct1, ct2, L), f"{name} tensor_prod_2x2 case {i}", pl)
        buf = P.to_device(np.concatenate([ct1, np.zeros((1, L, n), dtype=np.uint64)]), gpu)
        ctx.tensor_square_2x2_rns_poly(buf, buf, L)
        first_diff_limb(P.to_host(buf), oc.tensor_square_2x2(ct1, L), f"{name} tensor_square_2x2 case {i}", pl)
        for v, w in zip((da, db, dd), (a, b, d)):
            assert np.array_equal(P.to_host(v), w), "an operand was written to"
    del ctx
    _release()


@pytest.mark.parametrize("name", ROW_SETS)
def test_c_sums_at_every_term_count(name, gpu):
    """pha_tensor_prod_2x2_sum_batched and pha_multiply_plain_sum_batched over every row of the set's table, batch 1, at every term
    count of TERMS: one run of terms uploaded once, a term count is a slice of it."""
    import torch
    P, oc, ctx, n, qp, size_p, size_q = _setup(name, gpu)
    L, kmax = len(qp), max(TERMS)
    ct_w, ln = 2 * L * n, L * n
    rng = _rng(name, "sums")
    op1, op2 = (M.planted(rng, qp, (kmax, 2), n) for _ in range(2))
    plain, acc = M.planted(rng, qp, (kmax,), n), M.planted(rng, qp, (1, 2), n)
    ref_t = M.tensor_sums(oc, op1, op2, L, set(TERMS))
    ref_p = M.plain_sums(oc, plain, op1, L, set(TERMS))
    d1, d2, dp, da = (P.to_device(v, gpu) for v in (op1, op2, plain, acc))
    keep = [v.clone() for v in (d1, d2, dp, da)]
    for terms in TERMS:
        r01, r2 = _poisoned((1, 2, L, n), gpu), _poisoned((1, L, n), gpu)
        ctx.tensor_prod_2x2_sum_batched(d1, d2, r01, r2, L, terms, 1, strides=(ct_w, ct_w, ct_w, ct_w))
        first_diff_limb(P.to_host(r01)[0], ref_t[terms][:2], f"{name} tensor sum terms={terms} (c0, c1)", qp)
        first_diff_limb(P.to_host(r2)[0], ref_t[terms][2], f"{name} tensor sum terms={terms} c2", qp)
        for with_acc in (False, True):
            res = _poisoned((1, 2, L, n), gpu)
            ctx.multiply_plain_sum_batched(dp, d1, da if with_acc else None, res, L, terms, 1, strides=(ln, ln, ct_w, ct_w, ct_w))
            want = M.add_ct(oc, acc[0], ref_p[terms], L) if with_acc else ref_p[terms]
            first_diff_limb(P.to_host(res)[0], want, f"{name} plain sum terms={terms} acc={with_acc}", qp)
    assert all(torch.equal(a, b) for a, b in zip((d1, d2, dp, da), keep)), "a sum wrote to an operand"
    del ctx, d1, d2, dp, da, keep
    _release()


# ---- D ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,levels", KS_LEVELS, ids=[c[0] for c in KS_LEVELS])
def test_d_conversions_and_key_switch(name, levels, gpu):
    P, oc, ctx, n, qp, size_p, size_q = _setup(name, gpu, BGV_T)
    r = _rng(name, "ks")
    evk = _keys(r, qp, n, size_q, size_p)
    rlk = P.PhantomRelinKey.from_numpy(evk, gpu)
    batch = 3
    for ql in levels:
        tool = O.Tool(oc, ql)
        beta, qlp = tool.beta, ql + size_p
        pl, plp = qp[:ql], qp[:ql] + qp[size_q:]
        keys = [evk[i] for i in range(beta)]
        assert ctx.beta(ql) == beta
        cts, c2s = _cts(r, pl, n, batch), _cts(r, pl, n, batch, polys=1)[:, 0]
        for b in range(2):                                   # mod-up and mod-down: the all-(q - 1) polynomial and a uniform one
            d_mu = _poisoned((beta, qlp, n), gpu)
            d_c2 = P.to_device(c2s[b], gpu)
            ctx.modup(ql, d_mu, d_c2, O.CKKS)
            ref_mu = tool.modup(c2s[b], O.CKKS)
            for d in range(beta):
                first_diff_limb(P.to_host(d_mu)[d], ref_mu[d], f"{name} modup level {ql} digit {d} input {b}", plp)
            assert np.array_equal(P.to_host(d_c2), c2s[b])
            cx = ref_mu[beta - 1]                            # any [Ql || P] polynomial in NTT form
            d_cx, d_out = P.to_device(cx, gpu), _poisoned((ql, n), gpu)
            ctx.moddown_from_NTT(ql, d_out, d_cx, O.CKKS)
            first_diff_limb(P.to_host(d_out), tool.moddown_from_ntt(cx, O.CKKS), f"{name} moddown level {ql} input {b}", pl)
        src = M.edge_inputs(r, qp[size_q:], n)
        for kind in range(3):
            dst = _poisoned((ql, n), gpu)
            ctx.bconv_P_to_Ql(ql, dst, P.to_device(src[kind], gpu))
            first_diff_limb(P.to_host(dst), O.bconv(qp[size_q:], pl, src[kind], n), f"{name} bconv_P_to_Ql level {ql} input {kind}", pl)
        # the key switch: single, batched, fused with the rescale (single and batched)
        refs = [tool.keyswitch_inplace(cts[b], c2s[b], keys, O.CKKS) for b in range(batch)]
        for b in range(2):
            d_ct = P.to_device(cts[b], gpu)
            ctx.keyswitch_inplace(ql, d_ct, P.to_device(c2s[b], gpu), rlk.public_keys_ptr, O.CKKS)
            first_diff_limb(P.to_host(d_ct), refs[b], f"{name} keyswitch_inplace level {ql} ciphertext {b}", pl)
        d_ct, d_c2 = P.to_device(cts, gpu), P.to_device(c2s, gpu)
        ctx.keyswitch_inplace_batched(ql, d_ct, d_c2, batch, rlk.public_keys_ptr, O.CKKS)
        for b in range(batch):
            first_diff_limb(P.to_host(d_ct)[b], refs[b], f"{name} keyswitch_inplace_batched level {ql} ciphertext {b}", pl)
        assert np.array_equal(P.to_host(d_c2), c2s)
        if ql > 1:
            res = [tool.rescale_ntt(refs[b], 2) for b in range(batch)]
            dst = _poisoned((2, ql - 1, n), gpu)
            ctx.divide_and_round_q_last_ntt(ql, P.to_device(refs[0], gpu), 2, dst)
            first_diff_limb(P.to_host(dst), res[0], f"{name} divide_and_round_q_last_ntt level {ql}", pl[:-1])
            d_ct = P.to_device(cts, gpu)
            for b in range(2):
                dst = _poisoned((2, ql - 1, n), gpu)
                ctx.keyswitch_rescale(ql, d_ct[b], d_c2[b], rlk.public_keys_ptr, dst)
                first_diff_limb(P.to_host(dst), res[b], f"{name} keyswitch_rescale level {ql} ciphertext {b}", pl[:-1])
            dst = _poisoned((batch, 2, ql - 1, n), gpu)
            ctx.keyswitch_rescale_batched(ql, d_ct, d_c2, batch, rlk.public_keys_ptr, dst)
            for b in range(batch):
                first_diff_limb(P.to_host(dst)[b], res[b], f"{name} keyswitch_rescale_batched level {ql} ciphertext {b}", pl[:-1])
            # the key switch fused with the BGV modulus switch (single and batched) at the same digit shape
            bgv = O.Tool(oc, ql).set_plain_modulus(BGV_T)
            sw = [bgv.mod_t_divide_q_last_ntt(bgv.keyswitch_inplace(cts[b], c2s[b], keys, O.BGV), 2) for b in range(batch)]
            for b in range(2):
                dst = _poisoned((2, ql - 1, n), gpu)
                ctx.keyswitch_mod_switch(ql, d_ct[b], d_c2[b], rlk.public_keys_ptr, dst)
                first_diff_limb(P.to_host(dst), sw[b], f"{name} keyswitch_mod_switch level {ql} ciphertext {b}", pl[:-1])
            dst = _poisoned((batch, 2, ql - 1, n), gpu)
            ctx.keyswitch_mod_switch_batched(ql, d_ct, d_c2, batch, rlk.public_keys_ptr, dst)
            for b in range(batch):
                first_diff_limb(P.to_host(dst)[b], sw[b], f"{name} keyswitch_mod_switch_batched level {ql} ciphertext {b}", pl[:-1])
            assert np.array_equal(P.to_host(d_ct), cts) and np.array_equal(P.to_host(d_c2), c2s), "a fused entry wrote to its operands"
    del ctx, rlk
    _release()


def test_d_hoisting_weighted_three_elements(gpu):
    name, ql = "edge12", 8
    P, oc, ctx, n, qp, size_p, size_q = _setup(name, gpu)
    tool = O.Tool(oc, ql)
    r = _rng(name, "hoist")
    elts = [1] + [int(pow(5, i + 1, 2 * n)) for i in range(2)]
    glk_rot = [_keys(r, qp, n, size_q, size_p) for _ in elts[1:]]
    plp = qp[:ql] + qp[size_q:]
    weights = [uniform_poly(r, plp, n) for _ in elts]
    weights[0][:] = np.array(plp, dtype=np.uint64)[:, None] - np.uint64(1)
    dev_keys = [None] + [P.PhantomRelinKey.from_numpy(k, gpu) for k in glk_rot]
    glk = [None] + [[k[i] for i in range(tool.beta)] for k in glk_rot]
    ct = _cts(r, qp[:ql], n, 1)[0]
    d_ct = P.to_device(ct, gpu)
    ctx.hoisting_weighted(ql, d_ct, elts, dev_keys, [P.to_device(w, gpu) for w in weights], O.CKKS)
    first_diff_limb(P.to_host(d_ct), tool.hoisting_weighted(ct, elts, glk, weights, O.CKKS), f"{name} hoisting_weighted", qp[:ql])
    del ctx, dev_keys
    _release()


# ---- E ---------------------------------------------------------------------------------------------------------------------------------
def _bgv_moduli(name, level):
    """(label, t) of the BGV cases: every plain modulus below the smallest live limb, and on edge12 T59 (below the 60-bit limb only)."""
    qp = M.primes_of(name)[1]
    out = [(lb, M.plain_modulus(name, lb)) for lb in ("2", "257", "40961", "t40", "below") if M.plain_modulus(name, lb) < min(qp[:level])]
    return out + ([("T59", M.T59)] if name == "edge12" else [])


@pytest.mark.parametrize("name,levels", [("edge12", (8, 3)), ("small12", (6, 3))], ids=["edge12", "small12"])
def test_e_bgv_switches_decryption_and_budget(name, levels, gpu):
    import torch
    k = M.keyed(name)
    for label, t in _bgv_moduli(name, max(levels)):
        P, oc, ctx, n, qp, size_p, size_q = _setup(name, gpu, t)
        r = _rng(name, "bgv", label)
        evk = _keys(r, qp, n, size_q, size_p)
        rlk = P.PhantomRelinKey.from_numpy(evk, gpu)
        sk = ctx.secret_key_powers(P.to_device(k.sk_ntt, gpu), 2)
        for ql in levels:
            if t >= min(qp[:ql]) and label != "T59":
                continue
            what = f"{name} t={label} level {ql}"
            tool = O.Tool(oc, ql).set_plain_modulus(t)
            pl, keys = qp[:ql], [evk[i] for i in range(tool.beta)]
            cts, c2s = _cts(r, pl, n, 3), _cts(r, pl, n, 3, polys=1)[:, 0]
            # the modulus switch alone, then fused behind the key switch (single and batched)
            dst = _poisoned((2, ql - 1, n), gpu)
            ctx.mod_t_and_divide_q_last_ntt(ql, P.to_device(cts[1], gpu), 2, dst)
            first_diff_limb(P.to_host(dst), tool.mod_t_divide_q_last_ntt(cts[1], 2), f"{what} mod_t_and_divide_q_last_ntt", pl[:-1])
            dst = _poisoned((2, ql - 1, n), gpu)
            ctx.mod_t_and_divide_q_last_ntt(ql, P.to_device(cts[0], gpu), 2, dst)
            first_diff_limb(P.to_host(dst), tool.mod_t_divide_q_last_ntt(cts[0], 2), f"{what} mod_t_and_divide_q_last_ntt at q - 1", pl[:-1])
            refs = [tool.mod_t_divide_q_last_ntt(tool.keyswitch_inplace(cts[b], c2s[b], keys, O.BGV), 2) for b in range(3)]
            d_ct, d_c2 = P.to_device(cts, gpu), P.to_device(c2s, gpu)
            for b in range(2):
                dst = _poisoned((2, ql - 1, n), gpu)
                ctx.keyswitch_mod_switch(ql, d_ct[b], d_c2[b], rlk.public_keys_ptr, dst)
                first_diff_limb(P.to_host(dst), refs[b], f"{what} keyswitch_mod_switch ciphertext {b}", pl[:-1])
            dst = _poisoned((3, 2, ql - 1, n), gpu)
            ctx.keyswitch_mod_switch_batched(ql, d_ct, d_c2, 3, rlk.public_keys_ptr, dst)
            for b in range(3):
                first_diff_limb(P.to_host(dst)[b], refs[b], f"{what} keyswitch_mod_switch_batched ciphertext {b}", pl[:-1])
            assert np.array_equal(P.to_host(d_ct), cts) and np.array_equal(P.to_host(d_c2), c2s)
            # two fresh ciphertexts: decryption and noise budget against the restatement and Python integers
            m = k.messages(t, 2, tag=("bgv", ql))
            fresh = np.stack([k.encrypt(O.BGV, t, m[i], ql, ("bgv", ql, i)) for i in range(2)])
            d_fresh = P.to_device(fresh, gpu)
            out = _poisoned((2, n), gpu)
            ctx.bgv_decrypt_batched(ql, d_fresh, sk, out)
            budget, norm = _poisoned((2,), gpu, torch.int32), _poisoned((2, ql), gpu)
            ctx.invariant_noise_budget_batched(ql, d_fresh, sk, P.scheme_type.bgv, budget, norm)
            got, got_norm = P.to_host(out), P.to_host(norm)
            for i in range(2):
                plain, margin, worst, big = k.decrypt(O.BGV, t, fresh[i], ql, with_norm=True)
                assert np.array_equal(plain, m[i]) and margin >= MIN_MARGIN, what
                assert np.array_equal(got[i], m[i]), f"{what}: bgv_decrypt_batched ciphertext {i}"
                assert [int(w) for w in got_norm[i]] == [(worst >> (64 * w)) & (2 ** 64 - 1) for w in range(ql)], f"{what}: norm {i}"
                assert int(budget[i]) == max(0, big.bit_length() - worst.bit_length() - 1), f"{what}: budget {i}"
            assert np.array_equal(P.to_host(d_fresh), fresh)
        del ctx, rlk, sk
        _release()


# ---- F ---------------------------------------------------------------------------------------------------------------------------------
def _single(ctx, variant, a, b, dst):
    {"behz": ctx.bfv_multiply_behz, "hps": ctx.bfv_multiply_hps, "overq": ctx.bfv_multiply_hps_overq}[variant](a, b, dst)


def _batched(ctx, variant, d1, d2, dst, size_q):
    if variant == "overq":
        ctx.bfv_multiply_hps_overq_batched(size_q, d1, d2, dst)
    else:
        {"behz": ctx.bfv_multiply_behz_batched, "hps": ctx.bfv_multiply_hps_batched}[variant](d1, d2, dst)


@pytest.mark.parametrize("name,label", list(M.BFV_CELLS), ids=[f"{n}-{l}" for n, l in M.BFV_CELLS])
def test_f_bfv_cells(name, label, gpu):
    import torch
    k = M.keyed(name)
    t, m, cts, want = M.bfv_operands(name, label)
    P, oc, ctx, n, qp, size_p, size_q = _setup(name, gpu, t)
    pl = qp[:size_q]
    # pair 0: the two encryptions; pair 1: swapped, so that the second ciphertext of a batch differs from the first
    ct1, ct2 = np.stack([cts[0], cts[1]]), np.stack([cts[1], cts[0]])
    d1, d2 = P.to_device(ct1, gpu), P.to_device(ct2, gpu)
    for variant in M.VARIANTS:
        status, reason = M.cell_status(name, label, variant)
        if status != M.IN:
            print(f"{name} t={label} {variant}: {status} ({reason}); see test_g_* and tests/test_modulus_shapes.py")
            continue
        what = f"{name} t={label} {variant}"
        mul = M.multiplier(variant, oc, t)
        refs = [mul.multiply(ct1[b], ct2[b]) for b in range(2)]
        one = _poisoned((3, size_q, n), gpu)
        _single(ctx, variant, d1[0], d2[0], one)
        first_diff_limb(P.to_host(one), refs[0], f"{what} single entry", pl)
        dst = _poisoned((2, 3, size_q, n), gpu)
        _batched(ctx, variant, d1, d2, dst, size_q)
        got = P.to_host(dst)
        for b in range(2):
            first_diff_limb(got[b], refs[b], f"{what} batched entry ciphertext {b}", pl)
            plain, margin = k.decrypt(O.BFV, t, got[b], size_q)
            print(f"{what}: GPU product {b} margin {margin:.1f} bits")
            assert np.array_equal(plain, want), f"{what}: the GPU product {b} decrypts to something else"      # a b = b a
            assert margin >= MIN_MARGIN, f"{what}: margin {margin:.1f}"
    assert np.array_equal(P.to_host(d1), ct1) and np.array_equal(P.to_host(d2), ct2), "a multiply wrote to its operands"
    # decryption and noise budget of the fresh operands
    sk = ctx.secret_key_powers(P.to_device(k.sk_ntt, gpu), 2)
    out, budget, norm = _poisoned((2, n), gpu), _poisoned((2,), gpu, torch.int32), _poisoned((2, size_q), gpu)
    ctx.bfv_decrypt_batched(size_q, d1, sk, out)
    ctx.invariant_noise_budget_batched(size_q, d1, sk, P.scheme_type.bfv, budget, norm)
    for i in range(2):
        plain, margin, worst, big = k.decrypt(O.BFV, t, ct1[i], size_q, with_norm=True)
        assert np.array_equal(plain, m[i])
        assert np.array_equal(P.to_host(out)[i], m[i]), f"{name} t={label}: bfv_decrypt_batched ciphertext {i}"
        assert [int(w) for w in P.to_host(norm)[i]] == [(worst >> (64 * w)) & (2 ** 64 - 1) for w in range(size_q)], f"{name} t={label}: norm {i}"
        assert int(budget[i]) == max(0, big.bit_length() - worst.bit_length() - 1), f"{name} t={label}: budget {i}"
    # one level down: hps_overq_leveled and its fusion with the relinearization
    if name in ("low50", "low60"):
        ql = size_q - 1
        hq, tool = O.HpsOverQ(oc, t, ql), O.Tool(oc, ql)
        ref = hq.multiply(ct1[0], ct2[0])
        one = _poisoned((3, size_q, n), gpu)
        ctx.bfv_multiply_hps_overq_leveled(ql, d1[0], d2[0], one)
        first_diff_limb(P.to_host(one), ref, f"{name} t={label} hps_overq_leveled", pl)
        plain, margin = k.decrypt(O.BFV, t, P.to_host(one), size_q)
        if (name, label) in M.LEVELED_OUT:
            print(f"{name} t={label} hps_overq_leveled: out-of-domain ({M.LEVELED_OUT[(name, label)]})")
        else:
            assert np.array_equal(plain, want) and margin >= MIN_MARGIN, f"{name} t={label} hps_overq_leveled: margin {margin:.1f}"
        evk = _keys(_rng(name, "relin", label), qp, n, size_q, size_p)
        rlk = P.PhantomRelinKey.from_numpy(evk, gpu)
        two = _poisoned((2, size_q, n), gpu)
        ctx.bfv_mul_relin_hps_overq_leveled(ql, d1[0], d2[0], rlk.public_keys_ptr, two)
        first_diff_limb(P.to_host(two), hq.mul_relin_leveled(tool, ct1[0], ct2[0], [evk[i] for i in range(tool.beta)]),
                        f"{name} t={label} bfv_mul_relin_hps_overq_leveled", pl)
        del rlk
    del ctx, sk
    _release()


# ---- G ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bottom50", "tiny12"])
def test_g_no_hps_base_is_refused_and_behz_goes_on(name, gpu):
    """The walk down from the smallest data prime to 2^(bits - 1) finds too few primes for base R: the reference's logic_error (status
    PHA_ERR_LOGIC = -2, ArithmeticError here) with its text, nothing written, and the same context then multiplies by BEHZ as the
    oracle does."""
    t = 40961
    k = M.keyed(name)
    P, oc, ctx, n, qp, size_p, size_q = _setup(name, gpu, t)
    for cls in (O.Hps, O.HpsOverQ):
        with pytest.raises(ValueError, match="cannot set up the HPS bases"):
            cls(oc, t)
    m = k.messages(t, 2)
    cts = np.stack([k.encrypt(O.BFV, t, m[i], size_q, ("refuse", i)) for i in range(2)])
    d = P.to_device(cts, gpu)
    dst = _poisoned((3, size_q, n), gpu)
    before = dst.clone()
    for fn in (ctx.bfv_multiply_hps, ctx.bfv_multiply_hps_overq):
        with pytest.raises(ArithmeticError, match="failed to find enough qualifying primes 2"):
            fn(d[0], d[1], dst)
    for fn in (ctx.bfv_multiply_hps_batched, lambda a, b, c: ctx.bfv_multiply_hps_overq_batched(size_q, a, b, c)):
        with pytest.raises(ArithmeticError, match="failed to find enough qualifying primes 2"):
            fn(d[:1], d[1:], dst[None])
    import torch
    stream = torch.cuda.current_stream().cuda_stream
    assert ctx._L.pha_bfv_multiply_hps(ctx._h, d[0].data_ptr(), d[1].data_ptr(), dst.data_ptr(), stream) == -2
    assert b"failed to find enough qualifying primes 2" in ctx._L.pha_last_error()
    torch.cuda.synchronize()
    assert bool((dst == before).all()), "a refused call wrote something"
    ctx.bfv_multiply_behz(d[0], d[1], dst)
    got = P.to_host(dst)
    first_diff_limb(got, O.Behz(oc, t).multiply(cts[0], cts[1]), f"{name} BEHZ after the refusals", qp[:size_q])
    plain, margin = k.decrypt(O.BFV, t, got, size_q)
    assert np.array_equal(plain, M.negacyclic_product(m[0], m[1], t)) and margin >= MIN_MARGIN
    del ctx
    _release()
