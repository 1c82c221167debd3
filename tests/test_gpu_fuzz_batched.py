"""Seeded random parameter sets through the summed and batched entries on the GPU, every ciphertext of every batch word for word
against the oracle.  The shape of test_gpu_fuzz.test_random_parameter_sets: one rng_for(SEED + case) draws everything, the failure
message prints the whole draw, PHA_FUZZ_EXTRA=k adds k more cases.  The case number modulo 3 is the scheme.  A draw is

  log_n in {12, 13, 14, 14}; alpha and dnum in 1 .. 4 (cases 27 and 28: alpha 2 with dnum 6 and 5, more than four digits);
  a prime size per limb out of SIZES (bfv: one size for all data limbs, as the HPS variants need, 60-bit special primes);
  the level ql in 1 .. |Q|; batch B in 1 .. 9; chunk out of {0, 1, 2, 3, B}; terms K in 1 .. 12; operand 2 / the plaintexts shared by
  the batch (batch stride 0) or not; acc or none; for bgv and bfv a plain modulus out of {65537, 786433, 2^16, 2^20}.

ckks: inner_product_relin_batched, inner_product_relin_rescale_batched (against keyswitch(sum) in the oracle, never the sum of key
      switches: section F of test_gpu_inner_product.py), plain_inner_product_rescale_batched, hoisting_batched,
      hoisting_weighted_batched, hoisting_weighted_bsgs_batched, hoisting_weighted_bsgs_blocks;
bgv:  keyswitch_mod_switch, keyswitch_mod_switch_batched, inner_product_relin_mod_switch_batched, multiply_plain_sum_batched,
      plain_inner_product_rescale_batched, the three hoisting forms;
bfv:  bfv_multiply_{behz, hps, hps_overq}_batched (hps_overq at the top level and at a random lower one),
      bfv_plain_inner_product_batched, hoisting_batched.

The references are the builders of the per-entry files (imported, not copied).  Every output is poisoned before the call and every
operand compared with its upload after the last call.  refusal(entry, draw) says, from the preconditions in include/phantom_amd.h,
which calls the library refuses: either the result equals the oracle's, or the call fails with status -1 (ValueError), the
documented message and an untouched output.  A refusal that refusal() does not predict is a failure.
tests/test_fuzz_batched_cases.py replays the draws without a device and checks what the default cases cover.
"""
import os

import numpy as np
import pytest

from oracle import oracle as O
from test_gpu_bfv_batched import _batched as _bfv_batched, _oracle as _bfv_oracle
from test_gpu_bgv_mod_switch import _oracle_fused
from test_gpu_hoisting_bsgs_batched import Setup as _BsgsSetup
from test_gpu_inner_product import _oracle_sum as _tensor_sum, _poisoned, _release
from test_gpu_plain_sum import _oracle_sum as _plain_sum
from util import first_diff_limb, oracle_bfv_plain_sum, rng_for

pytestmark = pytest.mark.gpu

SEED = 13160                            # (a base at which the default cases cover what tests/test_fuzz_batched_cases.py asks for)
CASES = list(range(30))
SIZES = [30, 36, 40, 41, 42, 43, 44, 45, 46, 47, 48, 49, 50, 51, 55, 59, 60]
PLAIN_MODULI = [65537, 786433, 1 << 16, 1 << 20]
SCHEMES = [O.CKKS, O.BGV, O.BFV]
MANY_DIGITS = {27: 6, 28: 5}            # case -> dnum at alpha 2: beta > 4 once for ckks, once for bgv
POISON = -0x2152411021524111

ENTRIES = {
    O.CKKS: ["inner_product_relin_batched", "inner_product_relin_rescale_batched", "plain_inner_product_rescale_batched", "hoisting_batched",
             "hoisting_weighted_batched", "hoisting_weighted_bsgs_batched", "hoisting_weighted_bsgs_blocks"],
    O.BGV: ["keyswitch_mod_switch", "keyswitch_mod_switch_batched", "inner_product_relin_mod_switch_batched", "multiply_plain_sum_batched",
            "plain_inner_product_rescale_batched", "hoisting_batched", "hoisting_weighted_batched", "hoisting_weighted_bsgs_batched"],
    O.BFV: ["bfv_multiply_behz_batched", "bfv_multiply_hps_batched", "bfv_multiply_hps_overq_batched", "bfv_multiply_hps_overq_batched leveled",
            "bfv_plain_inner_product_batched", "hoisting_batched"],
}


def draw(case, seed=SEED):
    """Everything case `case` runs with, and the generator that goes on to make its data."""
    rng = rng_for(seed + case)
    d = {"case": case, "scheme": SCHEMES[case % 3], "log_n": int(rng.choice([12, 13, 14, 14]))}
    d["alpha"], d["dnum"] = int(rng.integers(1, 5)), int(rng.integers(1, 5))
    if case in MANY_DIGITS:
        d["alpha"], d["dnum"] = 2, MANY_DIGITS[case]
    size_q = d["size_q"] = d["alpha"] * d["dnum"]
    if d["scheme"] == O.BFV:
        d["bits"] = [int(rng.choice(SIZES))] * size_q + [60] * d["alpha"]
    else:
        d["bits"] = [int(rng.choice(SIZES)) for _ in range(size_q + d["alpha"])]
    d["ql"] = int(rng.integers(1, size_q + 1))
    d["beta"] = -(-d["ql"] // d["alpha"])
    d["batch"] = int(rng.integers(1, 10))
    d["chunk"] = [0, 1, 2, 3, d["batch"]][int(rng.integers(0, 5))]
    d["terms"] = int(rng.integers(1, 13))
    d["shared"], d["acc"] = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
    d["t"] = int(rng.choice(PLAIN_MODULI)) if d["scheme"] != O.CKKS else None
    d["ql_low"] = int(rng.integers(1, size_q)) if d["scheme"] == O.BFV and size_q > 1 else None
    return d, rng


def refusal(entry, d):
    """None: the library computes `entry` for the draw; otherwise the message it refuses the call with (include/phantom_amd.h: the level
    drops need size_Ql >= 2; the baby-step / giant-step form stops at four key-switch digits; a leveled bfv multiply needs a level
    below |Q| to exist -- that one is not a refusal of the library: the test has nothing to call, reported as 'no lower level')."""
    if entry in ("inner_product_relin_rescale_batched", "plain_inner_product_rescale_batched") and d["ql"] < 2:
        return "cannot rescale the last remaining modulus"
    if entry in ("keyswitch_mod_switch", "keyswitch_mod_switch_batched", "inner_product_relin_mod_switch_batched") and d["ql"] < 2:
        return "cannot switch down the last remaining modulus"
    if entry in ("hoisting_weighted_bsgs_batched", "hoisting_weighted_bsgs_blocks") and d["beta"] > 4:
        return "more than 4 key-switch digits are not supported by the baby-step / giant-step form"
    if entry == "bfv_multiply_hps_overq_batched leveled" and d["ql_low"] is None:
        return "no lower level"
    return None


def _chain(rng, n, bits):
    """Distinct NTT primes of the sizes `bits` (largest first within a size, like CoeffModulus::Create)."""
    pools = {b: [int(p) for p in O.get_primes(n, b, bits.count(b))] for b in set(bits)}
    return [pools[b].pop(0) for b in bits]


class _Chain(_BsgsSetup):
    """test_gpu_hoisting_bsgs_batched.Setup (keys, weights, ciphertexts, the oracle's forms of them) on a drawn chain instead of a named one"""

    def __init__(self, d, primes, gpu):
        import phantom_fhe_amd as P
        self.P, self.gpu, self.scheme, self.ql = P, gpu, d["scheme"], d["ql"]
        self.log_n, self.primes, self.size_p = d["log_n"], primes, d["alpha"]
        self.n, self.size_q = 1 << d["log_n"], d["size_q"]
        self.oc = O.Ctx(self.log_n, primes, self.size_p)
        self.ctx = P.PhantomContext(self.log_n, primes, self.size_p, device=gpu)
        self.tool = O.Tool(self.oc, self.ql)
        if d["t"]:
            self.ctx.set_plain_modulus(d["t"])
            if d["scheme"] == O.BGV:
                self.tool.set_plain_modulus(d["t"])
        self.qlp_primes = [primes[i] for i in list(range(self.ql)) + [self.size_q + j for j in range(self.size_p)]]


class _Runner:
    """Runs one entry: computes and compares, or expects the refusal that refusal() predicts with the output left poisoned."""

    def __init__(self, d, primes):
        self.d, self.primes, self.ran, self.refused, self.seen = d, primes, [], [], []
        self.what = f"draw {d} primes {primes}"

    def __call__(self, entry, outs, call, refs):
        """outs: the poisoned outputs; call(): the library call; refs(): pairs (got, want, label, primes) for first_diff_limb"""
        import torch
        self.seen.append(entry)
        msg = refusal(entry, self.d)
        if msg == "no lower level":
            self.refused.append(entry + " (no lower level)")
            return
        if msg is None:
            try:
                call()
            except ValueError as e:
                raise AssertionError(f"{entry} was refused ({e}) although its preconditions hold; {self.what}") from e
            for got, want, label, primes in refs():
                first_diff_limb(got, want, f"{entry} {label}; {self.what}", primes)
            self.ran.append(entry)
            return
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == msg, f"{entry} refused with {str(e.value)!r}, not with {msg!r}; {self.what}"
        torch.cuda.synchronize()
        assert all(bool((o == POISON).all()) for o in outs), f"the refused {entry} wrote to its output; {self.what}"
        self.refused.append(entry)


def _uniform(rng, primes, lead, n):
    out = np.empty(tuple(lead) + (len(primes), n), dtype=np.uint64)
    for j, q in enumerate(primes):
        out[..., j, :] = rng.integers(0, int(q), tuple(lead) + (n,), dtype=np.uint64)
    return out


def run_case(case, gpu, seed=SEED):
    import torch
    d, rng = draw(case, seed)
    n, ql, B, K, chunk, scheme, t = 1 << d["log_n"], d["ql"], d["batch"], d["terms"], d["chunk"], d["scheme"], d["t"]
    primes = _chain(rng, n, d["bits"])
    s = _Chain(d, primes, gpu)
    P, ctx, oc, tool = s.P, s.ctx, s.oc, s.tool
    pl = primes[:ql]
    run = _Runner(d, primes)
    lead2 = (K,) if d["shared"] else (B, K)
    host, dev = {}, {}

    def up(name, arr):
        host[name], dev[name] = arr, P.to_device(arr, gpu)
        return dev[name]

    def per_ct(got_dev, want_of, limbs):
        got = P.to_host(got_dev)
        return [(got[b], want_of(b), f"ciphertext {b} of {B}", limbs) for b in range(B)]

    if scheme != O.BFV:
        evk = s.host_key(rng)
        rlk = P.PhantomRelinKey.from_numpy(evk, gpu)
        keys = [evk[i] for i in range(tool.beta)]
        kp = rlk.public_keys_ptr
        op1 = up("op1", _uniform(rng, pl, (B, K, 2), n))
        op2 = up("op2", _uniform(rng, pl, lead2 + (2,), n))
        plain = up("plain", _uniform(rng, pl, lead2, n))
        acc = up("acc", _uniform(rng, pl, (B, 2), n))
        c2 = up("c2", _uniform(rng, pl, (B,), n))
        a = acc if d["acc"] else None
        h = host
        g2 = (lambda b: h["op2"]) if d["shared"] else (lambda b: h["op2"][b])
        gp = (lambda b: h["plain"]) if d["shared"] else (lambda b: h["plain"][b])
        memo = {}

        def ks_of_sum(b):                   # keyswitch(sum), one per group, shared by the entries that start from it
            if b not in memo:
                sm = _tensor_sum(oc, h["op1"][b], g2(b), ql)
                memo[b] = tool.keyswitch_inplace(sm[:2], sm[2], keys, scheme)
            return memo[b]

        def psum(b):
            return _plain_sum(oc, gp(b), h["op1"][b], ql, acc=h["acc"][b] if d["acc"] else None)

        drop = (lambda x: tool.rescale_ntt(x, 2)) if scheme == O.CKKS else (lambda x: tool.mod_t_divide_q_last_ntt(x, 2))
        if scheme == O.CKKS:
            dst = _poisoned((B, 2, ql, n), gpu)
            run("inner_product_relin_batched", [dst], lambda: ctx.inner_product_relin_batched(ql, op1, op2, K, B, kp, scheme, dst, chunk=chunk),
                lambda: per_ct(dst, ks_of_sum, pl))
            dres = _poisoned((B, 2, max(ql - 1, 1), n), gpu)
            run("inner_product_relin_rescale_batched", [dres], lambda: ctx.inner_product_relin_rescale_batched(ql, op1, op2, K, B, kp, dres, chunk=chunk),
                lambda: per_ct(dres, lambda b: drop(ks_of_sum(b)), pl[:-1]))
        else:
            ct0 = op1[:, 0].contiguous()
            one = _poisoned((2, max(ql - 1, 1), n), gpu)
            run("keyswitch_mod_switch", [one], lambda: ctx.keyswitch_mod_switch(ql, ct0[B - 1], c2[B - 1], kp, one),
                lambda: [(P.to_host(one), _oracle_fused(tool, h["op1"][B - 1, 0], h["c2"][B - 1], keys), f"ciphertext {B - 1}", pl[:-1])])
            dms = _poisoned((B, 2, max(ql - 1, 1), n), gpu)
            run("keyswitch_mod_switch_batched", [dms], lambda: ctx.keyswitch_mod_switch_batched(ql, ct0, c2, B, kp, dms),
                lambda: per_ct(dms, lambda b: _oracle_fused(tool, h["op1"][b, 0], h["c2"][b], keys), pl[:-1]))
            dip = _poisoned((B, 2, max(ql - 1, 1), n), gpu)
            run("inner_product_relin_mod_switch_batched", [dip],
                lambda: ctx.inner_product_relin_mod_switch_batched(ql, op1, op2, K, B, kp, dip, chunk=chunk),
                lambda: per_ct(dip, lambda b: drop(ks_of_sum(b)), pl[:-1]))
            dsum = _poisoned((B, 2, ql, n), gpu)
            run("multiply_plain_sum_batched", [dsum], lambda: ctx.multiply_plain_sum_batched(plain, op1, a, dsum, ql, K, B),
                lambda: per_ct(dsum, psum, pl))
        dpl = _poisoned((B, 2, max(ql - 1, 1), n), gpu)
        run("plain_inner_product_rescale_batched", [dpl], lambda: ctx.plain_inner_product_rescale_batched(ql, plain, op1, a, K, B, scheme, dpl, chunk=chunk),
            lambda: per_ct(dpl, lambda b: drop(psum(b)), pl[:-1]))
        # the hoisting forms on the first term of every group: two keyed rotations, and a 2 x 2 split with the identity in both lists
        s.split(rng, 2, 2, True)
        cts, d_ct = h["op1"][:, 0], op1[:, 0].contiguous()
        rot, o_rot, d_rot = [s.baby[1], s.giant[1]], [s.o_bk[1], s.o_gk[1]], [s.d_bk[1], s.d_gk[1]]
        out = _poisoned((B, 2, ql, n), gpu)
        run("hoisting_batched", [out], lambda: ctx.hoisting_batched(ql, d_ct, rot, d_rot, scheme, out=out, chunk=chunk),
            lambda: per_ct(out, lambda b: tool.hoisting(cts[b], rot, o_rot, scheme), pl))
        outw = _poisoned((B, 2, ql, n), gpu)
        run("hoisting_weighted_batched", [outw],
            lambda: ctx.hoisting_weighted_batched(ql, d_ct, s.baby, s.d_bk, s.d_w[0], scheme, out=outw, chunk=chunk),
            lambda: per_ct(outw, lambda b: tool.hoisting_weighted(cts[b], s.baby, s.o_bk, s.h_w[0], scheme), pl))
        outb = _poisoned((B, 2, ql, n), gpu)
        run("hoisting_weighted_bsgs_batched", [outb], lambda: s.batched(d_ct, out=outb, chunk=chunk), lambda: per_ct(outb, lambda b: s.oracle(cts[b]), pl))
        if scheme == O.CKKS:
            # B row blocks that share the first ciphertext: block k takes the giant rows in the order (k, k + 1) mod 2
            blocks = [[s.d_w[(k + i) % 2] for i in range(2)] for k in range(B)]
            h_blocks = [[s.h_w[(k + i) % 2] for i in range(2)] for k in range(B)]
            outk = _poisoned((B, 2, ql, n), gpu)

            def block_ref(k):
                return tool.hoisting_weighted_bsgs(cts[0], s.baby, s.o_bk, s.giant, s.o_gk, h_blocks[k], scheme)

            run("hoisting_weighted_bsgs_blocks", [outk],
                lambda: ctx.hoisting_weighted_bsgs_blocks(ql, d_ct[0], s.baby, s.d_bk, s.giant, s.d_gk, blocks, outk, scheme),
                lambda: [(g, w, f"block {k} of {B}", pl) for k, (g, w) in enumerate(zip(P.to_host(outk), map(block_ref, range(B))))])
    else:
        size_q, pq = d["size_q"], primes[:d["size_q"]]
        ct1 = up("ct1", _uniform(rng, pq, (B, 2), n))
        ct2 = up("ct2", _uniform(rng, pq, (B, 2), n))
        for variant, entry, lvl in (("behz", "bfv_multiply_behz_batched", None), ("hps", "bfv_multiply_hps_batched", None),
                                    ("overq", "bfv_multiply_hps_overq_batched", None), ("overq", "bfv_multiply_hps_overq_batched leveled", d["ql_low"])):
            dst3 = _poisoned((B, 3, size_q, n), gpu)
            orc = _bfv_oracle(variant, oc, t, lvl) if refusal(entry, d) is None else None
            run(entry, [dst3], lambda: _bfv_batched(ctx, variant, ct1, ct2, dst3, size_q, lvl, chunk),
                lambda: per_ct(dst3, lambda b: orc.multiply(host["ct1"][b], host["ct2"][b]), pq))
        m = up("m", rng.integers(0, t, lead2 + (n,), dtype=np.uint64))
        cts = up("cts", _uniform(rng, pl, (B, K, 2), n))
        acc = up("acc", _uniform(rng, pl, (B, 2), n))
        gm = (lambda b: host["m"]) if d["shared"] else (lambda b: host["m"][b])
        res = _poisoned((B, 2, ql, n), gpu)
        run("bfv_plain_inner_product_batched", [res],
            lambda: ctx.bfv_plain_inner_product_batched(ql, m, cts, acc if d["acc"] else None, res, K, B, chunk=chunk),
            lambda: per_ct(res, lambda b: oracle_bfv_plain_sum(oc, gm(b), host["cts"][b], ql, t, acc=host["acc"][b] if d["acc"] else None), pl))
        s.split(rng, 2, 2, True)
        rot, o_rot, d_rot = [s.baby[1], s.giant[1]], [s.o_bk[1], s.o_gk[1]], [s.d_bk[1], s.d_gk[1]]
        h_ct, d_ct = host["cts"][:, 0], cts[:, 0].contiguous()
        out = _poisoned((B, 2, ql, n), gpu)
        run("hoisting_batched", [out], lambda: ctx.hoisting_batched(ql, d_ct, rot, d_rot, scheme, out=out, chunk=chunk),
            lambda: per_ct(out, lambda b: tool.hoisting(h_ct[b], rot, o_rot, scheme), pl))
    for name, arr in host.items():
        assert np.array_equal(P.to_host(dev[name]), arr), f"an entry wrote to its operand {name}; {run.what}"
    assert run.seen == ENTRIES[scheme], run.seen
    print(f"FUZZ_CASE {d} ran={run.ran} refused={run.refused}")
    del s, ctx, dev
    _release()
    torch.cuda.synchronize()


# PHA_FUZZ_EXTRA=k adds k more seeded cases (a longer hunt, not part of the default run)
@pytest.mark.parametrize("case", CASES + [100 + i for i in range(int(os.environ.get("PHA_FUZZ_EXTRA", "0")))])
def test_random_parameter_sets_batched(case, gpu):
    run_case(case, gpu)


def test_bfv_multiply_with_special_primes_of_the_data_size(gpu):
    """Named regression, the smallest form of what case 20 of the first seed base found: data and special primes of one size
    ([60, 60] + [60] at N = 2^12).  The base R of the HPS multiplies is the |Q| + 1 primes just below the smallest q_i, which then
    starts with the special prime; the context refused that repeat ("coeff_modulus is not coprime") although R only ever meets Q.
    All four multiplies against the oracle, batch 2."""
    import phantom_fhe_amd as P
    log_n, n, size_q, t, B = 12, 4096, 2, 65537, 2
    primes = [int(p) for p in O.coeff_modulus_create(n, [60, 60, 60])]
    oc = O.Ctx(log_n, primes, 1)
    ctx = P.PhantomContext(log_n, primes, 1, device=gpu)
    ctx.set_plain_modulus(t)
    rng = rng_for(SEED + 1000)
    h1, h2 = _uniform(rng, primes[:size_q], (B, 2), n), _uniform(rng, primes[:size_q], (B, 2), n)
    d1, d2 = P.to_device(h1, gpu), P.to_device(h2, gpu)
    for variant, lvl in (("hps", None), ("overq", None), ("overq", 1), ("behz", None)):
        dst = _poisoned((B, 3, size_q, n), gpu)
        _bfv_batched(ctx, variant, d1, d2, dst, size_q, lvl, 0)
        got, orc = P.to_host(dst), _bfv_oracle(variant, oc, t, lvl)
        for b in range(B):
            first_diff_limb(got[b], orc.multiply(h1[b], h2[b]), f"{variant} level {lvl or size_q} ciphertext {b}", primes[:size_q])
    assert np.array_equal(P.to_host(d1), h1) and np.array_equal(P.to_host(d2), h2)
    del ctx
    _release()
