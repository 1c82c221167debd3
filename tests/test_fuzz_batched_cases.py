"""What the default cases of tests/test_gpu_fuzz_batched.py cover, replayed without a device: the draws are seeded, so a change of the
seed base or of the draw that loses a corner fails here instead of quietly testing nothing.  Also the widths of the ladder chain that
tests/test_gpu_sum_widths.py is written for."""
from oracle import oracle as O
from test_gpu_fuzz_batched import CASES, ENTRIES, PLAIN_MODULI, SIZES, draw, refusal
from test_gpu_sum_widths import PLAIN_MAX, PLAIN_PERIODS, TENSOR_MAX, TENSOR_PERIODS, _straddle
from util import primes_of

DRAWS = [draw(case)[0] for case in CASES]


def _of(scheme):
    return [d for d in DRAWS if d["scheme"] == scheme]


def test_the_draws_are_reproducible_and_within_their_ranges():
    assert DRAWS == [draw(case)[0] for case in CASES]
    assert len(CASES) >= 30
    for d in DRAWS:
        assert d["scheme"] == [O.CKKS, O.BGV, O.BFV][d["case"] % 3]
        assert d["log_n"] in (12, 13, 14) and 1 <= d["alpha"] <= 4 and 1 <= d["dnum"] <= 6
        assert d["size_q"] == d["alpha"] * d["dnum"] and len(d["bits"]) == d["size_q"] + d["alpha"] and set(d["bits"]) <= set(SIZES)
        assert 1 <= d["ql"] <= d["size_q"] and d["beta"] == -(-d["ql"] // d["alpha"])
        assert 1 <= d["batch"] <= 9 and d["chunk"] in (0, 1, 2, 3, d["batch"]) and 1 <= d["terms"] <= 12
        assert (d["t"] in PLAIN_MODULI) == (d["scheme"] != O.CKKS)
        if d["scheme"] == O.BFV:
            assert len(set(d["bits"][:d["size_q"]])) == 1           # the HPS variants take one size of data prime
            assert d["t"] < 1 << (min(d["bits"]) - 1)               # the lift needs t below every q_i
    assert sum(d["log_n"] == 14 for d in DRAWS) * 3 >= len(DRAWS)


def test_every_scheme_sees_alpha_one_and_more():
    for scheme in (O.CKKS, O.BGV, O.BFV):
        assert any(d["alpha"] == 1 for d in _of(scheme)) and any(d["alpha"] > 1 for d in _of(scheme)), scheme


def test_the_corners_of_the_key_switch_occur():
    assert any(d["dnum"] == 1 for d in DRAWS)
    assert any(d["ql"] == 1 for d in DRAWS)
    assert any(d["ql"] % d["alpha"] for d in DRAWS), "no short last digit"
    assert any(d["beta"] > 4 for d in DRAWS)
    assert sorted(d["dnum"] for d in DRAWS if d["dnum"] > 4) == [5, 6]
    # special primes of the data primes' size: the base R of the HPS multiplies starts with them (the regression beside the fuzz)
    assert any(d["scheme"] == O.BFV and d["bits"][0] == 60 for d in DRAWS)
    for scheme in (O.CKKS, O.BGV):   # where the mod-up + inner product is fused (fusable_ip, pha_rns.hip)
        assert any(d["log_n"] == 14 and d["alpha"] > 1 and d["beta"] <= 4 for d in _of(scheme)), scheme


def test_every_width_class_has_a_live_data_limb():
    live = {b for d in DRAWS for b in d["bits"][:d["ql"]]}
    for lo, hi in ((0, 41), (42, 46), (47, 49), (50, 50), (51, 59), (60, 60)):
        assert any(lo <= b <= hi for b in live), (lo, hi)


def test_batch_chunk_and_sharing_vary():
    assert {d["batch"] % 4 for d in DRAWS} == {0, 1, 2, 3}
    assert any(d["chunk"] == 0 for d in DRAWS) and any(0 < d["chunk"] < d["batch"] for d in DRAWS)
    assert {d["shared"] for d in DRAWS} == {False, True}
    assert {d["acc"] for d in DRAWS} == {False, True}


def test_every_entry_computes_often_enough():
    """by the predicate of the GPU test: at least 8 of the default cases compute (are not refused) for every listed entry"""
    names = sorted({e for entries in ENTRIES.values() for e in entries})
    for entry in names:
        computed = sum(1 for d in DRAWS if entry in ENTRIES[d["scheme"]] and refusal(entry, d) is None)
        assert computed >= 8, (entry, computed)
    # and the refusals are exercised too
    assert any(refusal(e, d) not in (None, "no lower level") for d in DRAWS for e in ENTRIES[d["scheme"]])


def test_the_ladder_has_the_widths():
    log_n, primes, size_p = primes_of("ladder12")
    assert (log_n, size_p) == (12, 2) and len(set(primes)) == 16
    assert [int(q).bit_length() for q in primes] == [50, 49, 48, 47, 46, 45, 44, 42, 41, 51, 55, 59, 60, 60, 61, 61]
    assert max(_straddle(TENSOR_PERIODS)) + 2 <= TENSOR_MAX and max(_straddle(PLAIN_PERIODS)) + 2 <= PLAIN_MAX
    assert {2 * t for t in PLAIN_PERIODS + [101]} | {203} <= set(range(1, PLAIN_MAX + 1))
