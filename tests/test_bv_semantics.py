"""What the oracle's steps do to a BGV or BFV message, on exact integers: every case of tests/bv_semantics.py run through the oracle
pipeline (bv_semantics.Reference) on the CPU.  Each case decrypts to the integer answer in ALL N slots, with a margin of at least
MIN_MARGIN bits, and the integer answer differs from every listed wrong answer (opposite direction, unrotated, rows swapped, transpose,
BSGS weights without the roll-back, a missing, doubled or un-inverted BGV correction factor) in more than half of the slots.  The same
cases run on the GPU in tests/test_gpu_bv_semantics.py, whose margins may fall MARGIN_LOSS bits below the ones printed here
(profiles/bv_semantics.md has both columns)."""
import numpy as np
import pytest

import bv_semantics as S
from oracle import oracle as O

HALF12 = 2048

# (set, case, oracle implementation(s), arguments)
BGV_CASES = [
    (S.BGV12, "rotation", "rotate_many", (6, 1)), (S.BGV12, "rotation", "rotate_many", (6, 3)),
    (S.BGV12, "rotation", "rotate_many", (6, HALF12 - 1)), (S.BGV12, "rotation", "rotate_many", (6, None)),
    (S.BGV12, "rotation", "rotate_many", (6, 1, 3)), (S.BGV12, "rotation", "rotate_many", (3, 1)),
    (S.BGV14, "rotation", "rotate_many", (8, 1)),
    (S.BGV12, "products", "bgv_multiply_many", (6, 1)), (S.BGV12, "products", "bgv_multiply_many", (6, 1, True)),
    (S.BGV12, "products", "bgv_multiply_many", (6, 3)), (S.BGV12, "products", "bgv_multiply_many", (3, 1)),
    (S.BGV14, "products", "bgv_multiply_many", (8, 1)),
    (S.BGV12, "inner_product", "bgv_inner", (6, 3, 2, False)),
    (S.BGV12, "inner_product", "bgv_inner_switch", (6, 3, 2, False)), (S.BGV12, "inner_product", "bgv_inner_switch", (6, 3, 2, True)),
    (S.BGV12, "plain_sum", "bgv_plain_sum", (6, 3, 2, False)), (S.BGV12, "plain_sum", "bgv_plain_sum", (6, 3, 2, True)),
    (S.BGV12, "hoisting", "hoist_many", (6, (1, 2, 5), 1)), (S.BGV12, "hoisting", "hoist_many", (6, (1, 2, 5), 3)),
    (S.BGV12, "matvec", "matvec_many", (6, 8, 1)), (S.BGV12, "matvec", "matvec_many", (6, 8, 2)),
    (S.BGV12, "bsgs", "bsgs_many", (6, 4, 2, 1)), (S.BGV12, "bsgs", "bsgs_many", (6, 4, 2, 2)),
    (S.BGV12, "bsgs_blocks", "bsgs_blocks", (6, 4, 2, 3)),
    (S.BGV12, "relin_rotate", "bgv_relin_rotate_many", (6, 3)),
    (S.BGV12, "depth_two", ("+", "bgv_multiply_many", "mod_switch"), (6,)),
]
BFV_CASES = [
    (S.BFV12, "rotation", "rotate_many", (2, 1)), (S.BFV12, "rotation", "rotate_many", (2, 3)),
    (S.BFV12, "rotation", "rotate_many", (2, HALF12 - 1)), (S.BFV12, "rotation", "rotate_many", (2, None)),
    (S.BFV12, "hoisting", "hoist_many", (2, (1, 2, 5), 1)), (S.BFV12, "hoisting", "hoist_many", (2, (1, 2, 5), 3)),
    (S.BFV12, "products", ("bfv_multiply_many", "behz"), (2, 1)), (S.BFV12, "products", ("bfv_multiply_many", "behz"), (2, 1, True)),
    (S.BFV12, "products", ("bfv_multiply_many", "behz"), (2, 3)),
    (S.BFV12, "relin_rotate", "bfv_relin_rotate_many", (2, 3)),
    (S.BFV13, "products", ("bfv_multiply_many", "hps"), (4, 1)), (S.BFV13, "products", ("bfv_multiply_many", "hps"), (4, 2)),
    (S.BFV13, "products", ("bfv_multiply_many", "overq"), (4, 1)), (S.BFV13, "products", ("bfv_multiply_many", "overq"), (4, 1, True)),
    (S.BFV13, "products", ("bfv_multiply_many", "overq"), (4, 2)),
    (S.BFV13, "products", ("bfv_multiply_leveled", 3, False), (4, 1)), (S.BFV13, "products", ("bfv_multiply_leveled", 3, True), (4, 1)),
    (S.BFV13, "products", ("bfv_multiply_leveled", 3, False), (4, 2)),
    (S.BFV13, "depth_two", ("+", ("bfv_multiply_many", "hps"), None), (4,)),
    (S.BFV13, "depth_two", ("+", ("bfv_multiply_many", "overq"), None), (4,)),
]
TABLE = []


def _flat(x):
    return "_".join(_flat(y) for y in x if y != "+") if isinstance(x, tuple) else str(x)


def _id(c):
    return f"{c[0][0]}-{c[1]}-{_flat(c[2])}-{_flat(c[3])}"


@pytest.mark.parametrize("case", BGV_CASES + BFV_CASES, ids=_id)
def test_oracle_pipeline_is_exact_in_every_slot(case):
    (name, kind), fn, impls, args = case
    res = S.cpu(name, kind, fn, impls, *args)
    TABLE.append((_id(case), res.label, res.margin))
    print(f"{_id(case)}: {res.label}: margin {res.margin:.1f} bits, factor {res.factor}")
    S.check(res)
    if kind == O.BGV and (fn in ("products", "plain_sum", "depth_two") or "switch" in str(impls)):
        assert res.factor != 1 and len(res.factor_controls()) == 3, "a switched BGV result carries a factor (its wrong-factor controls ran)"


def test_bfv_plaintext_operations():
    name, kind = S.BFV12
    for res in S.cpu(name, kind, "bfv_plain_ops", "self", 2):
        TABLE.append((f"{name}-bfv_plain_ops", res.label, res.margin))
        print(f"{res.label}: margin {res.margin:.1f} bits")
        S.check(res)


@pytest.mark.parametrize("name,kind,tech", [S.BGV12 + (None,), S.BFV12 + ("behz",), S.BFV13 + ("hps",)])
def test_evaluator_level_operations(name, kind, tech):
    """The operations host/phantom.h offers, from oracle steps with the correction-factor rules as the helper states them."""
    for res in S.cpu_host(name, kind, tech):
        TABLE.append((f"{name}-host", res.label, res.margin))
        print(f"{res.label}: margin {res.margin:.1f} bits, factor {res.factor}")
        S.check(res)


def test_balance_finds_a_common_factor():
    for f1, f2 in [(9543, 54084), (54084, 61896), (1, 9543), (65536, 2), (12345, 12345)]:
        for common, e1, e2 in (S.balance(f1, f2), S.balance_centred(f1, f2)):
            assert e1 * f1 % S.T == e2 * f2 % S.T == common and e2 % S.T
        small = lambda e: min(e % S.T, S.T - e % S.T)
        (_, a1, a2), (_, b1, b2) = S.balance(f1, f2), S.balance_centred(f1, f2)
        # the remainder sequence holds a pair within a factor 2 of the true minimum, itself about 2 sqrt t
        assert small(b1) + small(b2) <= small(a1) + small(a2) <= 2 * (small(b1) + small(b2)) <= 4 * 2 * 256


def test_sums_of_different_factors_pay_for_uncentred_scalars():
    """add_inplace multiplies the balancing scalars in as residues in [0, t) (the reference, src/evaluate.cu:148-168, and the mirror):
    with the same pair centred the sum keeps several bits more.  Both decrypt exactly; the profile records the two margins."""
    as_is = {r.label: r for r in S.cpu_host(*S.BGV12)}
    centred = {r.label: r for r in S.cpu_host(*S.BGV12, None, True)}
    for label in ("add (different factors)", "sub (different factors)", "add_many (different factors)"):
        S.check(centred[label])
        TABLE.append(("hyb12_a2-host (centred scalars)", label, centred[label].margin))
        print(f"{label}: margin {as_is[label].margin:.1f} bits as the reference multiplies, {centred[label].margin:.1f} bits with centred scalars")
        assert centred[label].margin >= as_is[label].margin


# ---- the helper itself ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind,level", [S.BGV12 + (6,), S.BGV12 + (3,), S.BFV12 + (2,), S.BFV13 + (4,)])
def test_decrypt_of_encrypt_is_the_message(name, kind, level):
    sch = S.scheme(name, kind)
    z = S.messages(1, 1, sch.n)
    ct = S._enc(sch, S.CpuCodec(sch), z, level, "pin")[0]
    got, margin = sch.decode_ct(ct, level)
    assert np.array_equal(got, z[0]) and margin >= 20
    # the layout: slot i of row r is the plaintext evaluated at psi^(5^i) (row 0) and psi^-(5^i) (row 1); pinned on the definition by
    # tests/test_batch_restatement.py, here on the statement the cases rely on: X -> X^5 on the plaintext rotates both rows by 1
    plain = S.CpuCodec(sch).encode(z)[0]
    assert np.array_equal(sch.batch.decode(sch.batch.galois(plain, 5)), S.rot(z[0], 1))
    assert np.array_equal(sch.batch.decode(sch.batch.galois(plain, 2 * sch.n - 1)), S.swap(z[0]))


@pytest.mark.parametrize("name,kind,level", [S.BGV12 + (6,), S.BFV12 + (2,)])
def test_the_key_of_element_g_switches_s_of_x_to_the_g_to_s(name, kind, level):
    """c = (0, c1) under s(X^g) -- phase c1 s(X^g) -- key-switched with the helper's key of g has the same message under s: BGV
    keys carry noise scaled by t (without the scaling the message is wrong modulo t, the control)."""
    sch = S.scheme(name, kind)
    oc, g = sch.oc, 5
    z = S.messages(2, 1, sch.n)
    ct = S._enc(sch, S.CpuCodec(sch), z, level, "pin.key")[0]
    ref = S.Reference(sch)
    c0, c1 = ref.galois(ct[0], level, g), ref.galois(ct[1], level, g)          # decrypts under s(X^g) to m(X^g)
    out = sch.tool(level).keyswitch_inplace(np.stack([c0, np.zeros_like(c0)]), c1, sch.digits(g, level), kind)
    got, margin = sch.decode_ct(out, level)
    assert np.array_equal(got, S.rot(z[0], 1)) and margin >= 20
    if kind == O.BGV:
        plain = S.Scheme(name).oracle_key(g)            # ckks_semantics.Scheme's key from the same seed: noise not scaled by t
        bad = sch.tool(level).keyswitch_inplace(np.stack([c0, np.zeros_like(c0)]), c1, [plain[i] for i in range(sch.tool(level).beta)], kind)
        assert S.differ(sch.decode_ct(bad, level)[0], S.rot(z[0], 1)) > 0.5


def test_correction_factor_rules():
    """After one mod_t_divide_q_last_ntt the factor is q_last^-1 mod t; after a product of ciphertexts with factors f1 and f2 it is
    f1 f2."""
    name, kind = S.BGV12
    sch = S.scheme(name, kind)
    ref = S.Reference(sch)
    z = S.messages(3, 2, sch.n)
    a, b = S._enc(sch, S.CpuCodec(sch), z, 6, "pin.cf")
    a5, l5, f1 = ref.mod_switch(a, 6)
    assert l5 == 5 and f1 == pow(int(sch.primes[5]), -1, S.T)
    S.check(S.Result(sch, "switched", [a5], 5, z[:1], factor=f1))
    a4, l4, f2 = ref.mod_switch(a5, 5)
    assert f2 == pow(int(sch.primes[4]), -1, S.T) and f2 != f1
    S.check(S.Result(sch, "switched twice", [a4], 4, z[:1], factor=f1 * f2 % S.T))
    b5 = ref.mod_switch(b, 6)[0]
    prod = ref.relinearize(sch.oc.tensor_prod_2x2(a5, b5, 5), 5)
    S.check(S.Result(sch, "product of switched", [prod], 5, (z[0] * z[1] % S.TU)[None], factor=f1 * f1 % S.T))
    mixed = ref.relinearize(sch.oc.tensor_prod_2x2(a5, b[:, :5], 5), 5)       # b dropped to 5 limbs without a switch: factor 1
    S.check(S.Result(sch, "factors f1 and 1", [mixed], 5, (z[0] * z[1] % S.TU)[None], factor=f1))


def test_print_the_margins():
    """The left column of profiles/bv_semantics.md (run with -s)."""
    for row in TABLE:
        print("| %s | %s | %.1f |" % row)
