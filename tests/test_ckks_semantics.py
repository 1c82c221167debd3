"""What the oracle's operations do to a CKKS message (CPU only): numpy restatement encode -> oracle encrypt / Galois / key switch /
tensor product / hoisting / rescale -> restatement decode, compared with numpy on the slot vectors.  tests/test_oracle.py pins the
oracle by the meaning of its steps on coefficients; this file pins the slot conventions above them, once and on every machine:

* rotation step s <-> Galois element 5^s mod 2N <-> np.roll(z, -s) in the encoder's slot order; element 2N - 1 conjugates;
* sum_k diag_k o rotate_k(v) = M v for the diagonals of workloads.matrix_diagonals, and the baby-step / giant-step preparation
  np.roll(diag_{i n_baby + j}, +i n_baby) (ckks_semantics.bsgs_diagonals);
* products, inner products, plaintext-weighted sums, hoisted sums of rotations, relinearise + rotate, the NAF of a missing step.

Every case stays below 2^-16 (measured: at most 1e-6, see profiles/ckks_semantics.md) and is farther than 0.1 from every plausible
wrong answer.  The same cases, inputs and seeds run on the GPU in tests/test_gpu_ckks_semantics.py, bounded by the errors found here."""
import numpy as np
import pytest

import ckks_semantics as S

NAME, SCALE = "hyb12_a2", 2.0 ** 40


def _ref(name=NAME):
    sch = S.scheme(name)
    return sch, S.cpu_codec(name), S.Reference(sch, S.cpu_codec(name))


def _check(res):
    for r in res if isinstance(res, list) else [res]:
        print(f"{r.label}: error {r.err:.3e}, nearest wrong answer {r.wrong if r.wrong is None else round(r.wrong, 3)}")
        assert r.err < S.CPU_CAP, r.label
        assert r.wrong is None or r.wrong > S.FAR, r.label


def test_fresh_encryption_decrypts_to_the_message():
    sch, codec, _ = _ref()
    z = S.messages(1, 2, sch.slots)
    ct = S._enc(sch, codec, z, 6, SCALE, "fresh")
    _check(S.Result("fresh", S._dec(sch, codec, ct, 6, SCALE), z, [np.conj(z), np.roll(z, 1, axis=1)]))


def test_secret_key_under_an_automorphism_is_the_oracles():
    """s(X^elt) from index arithmetic equals the oracle's NTT-domain permutation of s: the two statements of the Galois map agree."""
    from oracle import oracle as O
    sch, _, _ = _ref()
    for elt in (5, 25, S.elt_of_step(-1, sch.n), 2 * sch.n - 1):
        want = O.apply_galois_ntt(sch.sk_ntt, O.galois_ntt_table(sch.log_n, elt), sch.n, sch.size_qp)
        assert np.array_equal(sch.sk_galois_ntt(elt), want), elt


def test_elements_of_steps_follow_the_reference_definition():
    """5^s mod 2N; a negative step -s is step slots - s (the reference's get_elt_from_step); NAF(3) = 4 - 1, NAF(5) = 4 + 1."""
    n = 4096
    assert S.elt_of_step(1, n) == 5 and S.elt_of_step(3, n) == 125 and S.elt_of_step(-1, n) == pow(5, n // 2 - 1, 2 * n)
    assert S.elt_of_step(1, n) * S.elt_of_step(-1, n) % (2 * n) == 1
    assert S.naf(3) == [-1, 4] and S.naf(5) == [1, 4] and S.naf(-3) == [1, -4] and S.naf(4) == [4] and S.naf(0) == []


@pytest.mark.parametrize("level", [6, 3])
@pytest.mark.parametrize("step", [1, 3, 2047, 1024, None])
def test_rotation(level, step):
    sch, codec, ref = _ref()
    _check(S.case_rotation(sch, codec, ref.rotate, level, SCALE, step))


@pytest.mark.parametrize("name,level,scale", [("hyb13_a3", 7, 2.0 ** 50), ("c2_ckks14", 8, 2.0 ** 40)])
def test_rotation_and_product_at_other_sets(name, level, scale):
    sch, codec, ref = _ref(name)
    _check(S.case_rotation(sch, codec, ref.rotate, level, scale, 1))
    _check(S.case_products(sch, codec, ref.multiply_many, level, scale, 1))


def test_products():
    sch, codec, ref = _ref()
    _check(S.case_products(sch, codec, ref.multiply_many, 6, SCALE, 3))
    _check(S.case_products(sch, codec, ref.multiply_many, 6, SCALE, 1, square=True))


@pytest.mark.parametrize("shared", [False, True])
def test_inner_product(shared):
    sch, codec, ref = _ref()
    _check(S.case_inner_product(sch, codec, ref.inner, 6, SCALE, 5, 2, shared))


@pytest.mark.parametrize("with_acc", [False, True])
def test_plain_sum(with_acc):
    sch, codec, ref = _ref()
    _check(S.case_plain_sum(sch, codec, ref.plain_sum, 6, SCALE, 4, 2, with_acc))


def test_hoisting():
    sch, codec, ref = _ref()
    _check(S.case_hoisting(sch, codec, ref.hoist_many, 6, SCALE, (1, 2, 5), 2))


@pytest.mark.parametrize("d", [8, 16])
def test_diag_matvec(d):
    sch, codec, ref = _ref()
    _check(S.case_matvec(sch, codec, ref.matvec_many, 5, SCALE, d, 3 if d == 8 else 1))


@pytest.mark.parametrize("n_baby,n_giant,batch", [(4, 2, 2), (4, 4, 1)])
def test_bsgs_matvec(n_baby, n_giant, batch):
    sch, codec, ref = _ref()
    _check(S.case_bsgs(sch, codec, ref.bsgs_many, 5, SCALE, n_baby, n_giant, batch))


def test_bsgs_row_blocks():
    sch, codec, ref = _ref()
    _check(S.case_bsgs_blocks(sch, codec, ref.bsgs_blocks, 5, SCALE, 4, 2, 2))


def test_bsgs_needs_the_roll_back():
    """The negative control is a real one: the diagonals without the roll-back give another vector, exactly the one numpy predicts."""
    sch, codec, ref = _ref()
    r = S.case_bsgs(sch, codec, ref.bsgs_many, 5, SCALE, 4, 2, 1, prepare=S.bsgs_diagonals_without_roll_back)
    print(f"without the roll-back: {r.err:.3f} from M v, {S.max_err(r.got, r.wrongs[-1]):.3e} from the prediction")
    assert r.err > S.FAR and S.max_err(r.got, r.wrongs[-1]) < S.CPU_CAP


def test_numpy_identities_of_the_diagonal_forms():
    """The two promises in numpy alone: sum_k diag_k o roll(v, -k) = M v, and the same through bsgs_diagonals."""
    slots = 64
    for d, nb in ((8, 4), (16, 4)):
        m = S.matrix(d, d, d)
        t, v = S.periodic(d, d, slots)
        want = np.tile(m @ v, slots // d)
        assert S.max_err(sum(dk * np.roll(t, -k) for k, dk in enumerate(S.matrix_diagonals(m, slots))), want) < 1e-12
        assert S.max_err(S.bsgs_apply(S.bsgs_diagonals(m, slots, nb, d // nb), t, nb), want) < 1e-12


def test_matrix_diagonals_of_the_library_are_the_tests():
    from phantom_fhe_amd import workloads as W
    m = S.matrix(3, 8, 8)
    assert np.array_equal(W.matrix_diagonals(m, 64), S.matrix_diagonals(m, 64))
    assert np.array_equal(W.matrix_diagonals(m, 64, [0, 3, 5]), S.matrix_diagonals(m, 64, [0, 3, 5]))


def test_config4_relinearize_rotate():
    sch, codec, ref = _ref()
    _check(S.case_config4(sch, codec, ref.relin_rotate_many, 6, SCALE, 3))


def test_config4_bfv_is_exact():
    c = S.BfvConfig4()
    for k1, k2 in ((0, 1), (0, 0)):
        assert c.decrypt(c.oracle(k1, k2)) == c.want(k1, k2)


def test_evaluator_operations_and_naf_rotations():
    sch, codec, ref = _ref()
    _check(S.case_host_api(sch, codec, S.ReferenceHost(ref, SCALE), SCALE))
