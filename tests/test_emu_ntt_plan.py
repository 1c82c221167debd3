"""Which kernels a launch shape takes (phantom-fhe_amd/csrc/pha_ntt_core.h: resolve_plan, and zloop_zper / zloop_fill behind it), pinned
on the CPU -- no GPU needed.  Harness: tests/emu/emu_ntt_plan.cpp (test-only).

Every plan of the NTT computes the same values, so a launch that takes another plan than the one it was tuned for still passes every
parity test.  The expected values here are NOT read off the code under test: sections A and B are the kernel traces recorded on an
MI355X in profiles/ntt_plan_switch_kernels.md (plan, tiles per limb and workgroup size of both passes; grid and polynomials per
workgroup of the twiddle-resident pass), the other cases are the rule text in front of resolve_plan.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from util import chain_bits

HERE = os.path.dirname(os.path.abspath(__file__))
NEVER = 1 << 30     # the experiments library's default thresholds (pha_ntt.hip: g_whole14_min, g_fused_min_tiles)
FIRST_ONLY, SECOND_ONLY, EXPERIMENTS, ROUND_ROBIN = 1, 2, 4, 8


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("emu_ntt_plan") / "libemu_ntt_plan.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fno-strict-aliasing", "-fPIC", "-shared", "-o", out,
                           os.path.join(HERE, "emu", "emu_ntt_plan.cpp")])
    L = C.CDLL(out)
    L.emu_ntt_plan.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_void_p]
    L.emu_ntt_plan.restype = C.c_int
    L.emu_ntt_plan_zloop.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    L.emu_ntt_plan_zloop.restype = C.c_int
    return L


def resolve(emu, log_n, limbs, batch, flags=0, bits=None, whole14_min=NEVER, one_launch_min_tiles=NEVER):
    out = np.zeros(8, dtype=np.uint32)
    bits = emu.emu_ntt_default_variant() if bits is None else bits
    rc = emu.emu_ntt_plan(log_n, limbs, batch, flags, bits, whole14_min, one_launch_min_tiles, out.ctypes.data)
    assert rc == 0, "NttPlan has no such plan"
    keys = ("plan", "whole", "zfast", "one_launch", "s_tiles", "s_threads", "c_tiles", "c_threads")
    r = dict(zip(keys, (int(v) for v in out)))
    r["one_launch_asked"], r["one_launch"] = r["one_launch"] >> 1, r["one_launch"] & 1
    return r


def zloop(emu, log_n, plan, batch, prime_bits):
    fp = np.array([1 if b <= 50 else 0 for b in prime_bits], dtype=np.uint8)
    out = np.zeros(2, dtype=np.uint32)
    assert emu.emu_ntt_plan_zloop(log_n, plan, len(prime_bits), batch, fp.ctypes.data, out.ctypes.data) == 0
    return int(out[0]), int(out[1])


def test_default_variant_is_the_one_the_gpu_tests_restore(emu):
    import test_gpu_ntt as G
    assert emu.emu_ntt_default_variant() == G.DEFAULT_VARIANT


# ---- section A of profiles/ntt_plan_switch_kernels.md: (log_n, limbs, batch, plan, strided pass (tiles per limb, threads), contiguous
# pass (tiles per limb, threads)).  Workgroup sizes as the table's legend names them: S 512 threads (256 on plan 10), C5 / C3 / C4 one
# wavefront, C10 128 threads, W13 one 512-thread workgroup per limb.
_A = [
    (13, 9, 7, 3, (2, 512), (16, 64)),
    (13, 8, 8, "W13", None, (1, 512)),
    (14, 64, 2, 5, (4, 512), (64, 64)),
    (14, 43, 3, 3, (4, 512), (32, 64)),
    (14, 51, 5, 3, (4, 512), (32, 64)),
    (14, 64, 4, 4, (4, 512), (32, 64)),
    (15, 16, 4, 5, (8, 512), (128, 64)),
    (15, 13, 5, 3, (8, 512), (64, 64)),
    (15, 63, 2, 3, (8, 512), (64, 64)),
    (15, 32, 4, 4, (8, 512), (64, 64)),
    (16, 16, 2, 5, (16, 512), (256, 64)),
    (16, 11, 3, 10, (32, 256), (64, 128)),
    (17, 31, 1, 3, (32, 512), (256, 64)),
    (17, 16, 2, 4, (32, 512), (256, 64)),
    # the single-polynomial rows
    (14, 64, 1, 5, (4, 512), (64, 64)),
    (15, 64, 1, 5, (8, 512), (128, 64)),
    (16, 32, 1, 5, (16, 512), (256, 64)),
    (16, 33, 1, 10, (32, 256), (64, 128)),
    (17, 32, 1, 4, (32, 512), (256, 64)),
    (14, 128, 1, 5, (4, 512), (64, 64)),
    (14, 129, 1, 3, (4, 512), (32, 64)),
    (15, 65, 1, 3, (8, 512), (64, 64)),
    (15, 127, 1, 3, (8, 512), (64, 64)),
    (15, 128, 1, 4, (8, 512), (64, 64)),
]


@pytest.mark.parametrize("log_n,limbs,batch,plan,strided,contiguous", _A, ids=[f"2^{c[0]}-{c[1]}x{c[2]}" for c in _A])
def test_section_a_both_sides_of_each_threshold(emu, log_n, limbs, batch, plan, strided, contiguous):
    r = resolve(emu, log_n, limbs, batch)
    assert not r["zfast"] and not r["one_launch"]
    if plan == "W13":
        assert r["whole"] == 13
    else:
        assert r["whole"] == 0 and r["plan"] == plan
        assert (r["s_tiles"], r["s_threads"]) == strided
    assert (r["c_tiles"], r["c_threads"]) == contiguous


# ---- section B: (log_n, batch, prime sizes of the selection, plan of the launch, grid of ntt_zloop_kernel, polynomials per workgroup);
# grid 0: the kernel is absent from the trace and the contiguous pass is the plan's own
_HALF_INT = (50, 60, 47, 55, 42, 60, 36, 55, 50, 60, 47, 55, 42, 60, 36, 55)
_HALF_INT_PLUS_ONE = (50, 60, 47, 55, 42, 60, 36, 55, 50, 60, 47, 55, 42, 60, 60, 55)
_WIDE = chain_bits(64, [50, 48, 47, 46, 43, 42, 41, 40, 36, 30]) + [61] * 65     # the wide context: 64 FP64 rows, then Bsk
_B = [
    ("2^14-16x32", 14, 32, chain_bits(16), 4, 6400, 4),
    ("2^14-32x16", 14, 16, chain_bits(32), 4, 6016, 4),
    ("2^15-32x8", 15, 8, chain_bits(32), 4, 6016, 4),
    ("2^16-16x8", 16, 8, chain_bits(16), 10, 3200, 4),
    ("2^17-8x8", 17, 8, chain_bits(8), 4, 5632, 4),
    ("2^16-16x12", 16, 12, chain_bits(16), 10, 5632, 3),
    ("2^16-32x17", 16, 17, chain_bits(32), 10, 10624, 6),
    ("B.1-limbs-3-19", 16, 8, chain_bits(20)[3:19], 10, 3200, 4),
    ("B.2-guard-limb-stride", 16, 8, chain_bits(16), 10, 3200, 4),
    ("B.3-half-integer", 16, 8, _HALF_INT, 10, 5120, 4),
    ("B.4-half-plus-one", 16, 8, _HALF_INT_PLUS_ONE, 10, 0, 0),
    ("B.5-128-limbs", 14, 8, _WIDE[:128], 4, 20480, 4),
    ("B.5-129-limbs", 14, 8, _WIDE[:129], 4, 0, 0),
]


@pytest.mark.parametrize("case", _B, ids=[c[0] for c in _B])
def test_section_b_resident_twiddle_grid(emu, case):
    _, log_n, batch, prime_bits, plan, grid, zper = case
    r = resolve(emu, log_n, len(prime_bits), batch)
    assert r["whole"] == 0 and r["plan"] == plan
    assert zloop(emu, log_n, plan, batch, prime_bits) == (zper, grid)


def test_section_b_contiguous_pass_where_the_resident_kernel_declines(emu):
    """B.4: C10 64 x 16 x 8; B.5 at 129 limbs: C4 32 x 129 x 8."""
    r = resolve(emu, 16, 16, 8)
    assert (r["plan"], r["c_tiles"], r["c_threads"]) == (10, 64, 128)
    r = resolve(emu, 14, 129, 8)
    assert (r["plan"], r["c_tiles"], r["c_threads"]) == (4, 32, 64)


# ---- the rule text ----------------------------------------------------------------------------------------------------------------
_SHAPES = [(1, 1), (3, 1), (9, 7), (8, 8), (45, 1), (45, 3), (45, 16), (64, 4), (128, 1), (16, 64)]
_ALL_BITS = [0, 1, 8, 9, 17, 25, 65, 73, 81, 225, 353, 361, 609, 617, 625, 1121, 2145, 6241, 10337, 18529]


@pytest.mark.parametrize("flags", [0, FIRST_ONLY], ids=["plain", "first-pass-only"])
def test_n_4096_is_one_launch_for_any_shape(emu, flags):
    for limbs, batch in _SHAPES:
        r = resolve(emu, 12, limbs, batch, flags)
        assert r["whole"] == 12 and not r["one_launch"]
        assert (r["c_tiles"], r["c_threads"]) == (1, 256)


def test_second_pass_only_keeps_the_two_pass_split_of_plan_3(emu):
    """The contiguous pass ran in the fused mod-up, on plan 3's T1 x T2: nothing above plan 5 (whose split is plan 3's), no
    one-workgroup plan, not the one-launch form -- whatever the tuning state."""
    for lib in (0, EXPERIMENTS | ROUND_ROBIN):
        for bits in (_ALL_BITS if lib else [6241]):
            for log_n in (13, 14, 15, 16, 17):
                for limbs, batch in _SHAPES:
                    r = resolve(emu, log_n, limbs, batch, lib | SECOND_ONLY, bits, whole14_min=1, one_launch_min_tiles=1)
                    assert r["plan"] <= 5 and r["whole"] == 0 and not r["one_launch"], (lib, bits, log_n, limbs, batch)


def test_halves_of_the_fused_mod_up_never_take_plan_10(emu):
    for flags in (FIRST_ONLY, SECOND_ONLY):
        for limbs, batch in _SHAPES:
            r = resolve(emu, 16, limbs, batch, flags)
            assert r["plan"] in (3, 4, 5), (flags, limbs, batch)
            assert resolve(emu, 16, limbs, batch, flags | EXPERIMENTS, 10337)["plan"] in (3, 4, 5)
    assert resolve(emu, 16, 45, 1)["plan"] == 10


@pytest.mark.parametrize("log_n,limbs,batch,want", [
    # tiles = N / 4096 x limbs x batch.  8191 is prime, so a launch of exactly 8191 tiles is one limb at N = 4096.
    (12, 1, 8191, False), (12, 1, 8192, True),
    (13, 511, 8, False), (13, 512, 8, True),            # 8176 / 8192 tiles of 8 polynomials
    (17, 32, 8, True), (17, 31, 8, False),              # 8192 / 7936
    (16, 64, 8, True), (16, 63, 8, False),              # 8192 / 8064
    (12, 1171, 7, False), (17, 37, 7, False), (16, 128, 7, False),   # 7 polynomials: 8197 / 8288 / 14336 tiles
], ids=lambda v: str(v))
def test_polynomial_fastest_order_from_8_polynomials_and_8192_tiles(emu, log_n, limbs, batch, want):
    assert bool(resolve(emu, log_n, limbs, batch)["zfast"]) == want


# ---- the experiments library's variant bits: the plan each id of tests/test_gpu_ntt.py names, at one two-pass shape per degree (the
# shapes of section A that lie past the small-launch rule and below 1024 tiles)
_DEGREE_SHAPE = {12: (3, 1), 13: (9, 7), 14: (43, 3), 15: (13, 5), 16: (11, 3), 17: (31, 1)}
# id -> plan per degree; "W": the one-workgroup plan of that degree; (plan, True): in the one-launch form
_ALL = (12, 13, 14, 15, 16, 17)
_NAMED = {
    "ept16": {d: 0 for d in _ALL}, "ept16-int": {d: 0 for d in _ALL},
    "ept8": {d: 1 for d in _ALL}, "ept8-int": {d: 1 for d in _ALL},
    "ept8-ot": {d: 2 for d in _ALL}, "ept8-ot-int": {d: 2 for d in _ALL},
    "ept8-wave": {d: 3 for d in _ALL}, "ept8-wave-int": {d: 3 for d in _ALL},
    "ept8-ot-wave": {d: 4 for d in _ALL},
    "two-pass-4096": {d: 3 for d in _ALL},
    "one-launch-8192-16384": {12: "W", 13: "W", 14: "W", 15: 3, 16: 3, 17: 3},
    "one-launch-8192-16384-int": {12: "W", 13: "W", 14: "W", 15: 3, 16: 3, 17: 3},
    "fused": {d: (3, True) for d in _ALL}, "fused-int": {d: (3, True) for d in _ALL}, "fused-ot": {d: (4, True) for d in _ALL},
    "never-fused": {d: 3 for d in _ALL},
    "r03-default": {d: 3 for d in _ALL},
    "default": {12: "W", 13: 3, 14: 3, 15: 3, 16: 10, 17: 3},
    "rows1024-one-wavefront": {12: "W", 13: 3, 14: 3, 15: 3, 16: 12, 17: 3},
    "split-128x512": {12: "W", 13: 3, 14: 3, 15: 3, 16: 8, 17: 3},
}
# N = 4096 runs its one-workgroup plan unless bit 7 ("two-pass-4096") sends it through the two-pass plans
for _name, _plans in _NAMED.items():
    if _name != "two-pass-4096":
        _plans[12] = "W"


def test_every_variant_of_the_gpu_sweep_resolves_to_the_plan_its_id_names(emu):
    import test_gpu_ntt as G
    assert sorted(G._VARIANT_IDS) == sorted(_NAMED) and G._VARIANTS == _ALL_BITS
    for bits, name in zip(G._VARIANTS, G._VARIANT_IDS):
        for log_n, (limbs, batch) in _DEGREE_SHAPE.items():
            want = _NAMED[name][log_n]
            # "never-fused" asks for the one-launch form at every size (threshold 1) and bit 10 must still refuse it
            r = resolve(emu, log_n, limbs, batch, EXPERIMENTS | ROUND_ROBIN, bits, one_launch_min_tiles=1 if name == "never-fused" else NEVER)
            got = "W" if r["whole"] else (r["plan"], True) if r["one_launch"] else r["plan"]
            assert got == want, (name, log_n, got, want)
            if r["whole"]:
                assert r["whole"] == log_n
    # the hand-off needs the round-robin placement: without it the same bits take two launches
    assert not resolve(emu, 15, 13, 5, EXPERIMENTS, 609)["one_launch"]
    # plan 10 has no one-launch form, but the request stays visible (the fused base conversion declines on it)
    r = resolve(emu, 16, 11, 3, EXPERIMENTS | ROUND_ROBIN, 609 | 4096)
    assert (r["plan"], r["one_launch"], r["one_launch_asked"]) == (10, 0, 1)
    assert not resolve(emu, 16, 11, 3, EXPERIMENTS | ROUND_ROBIN, 6241)["one_launch_asked"]


def test_product_library_ignores_the_experiments_only_inputs(emu):
    """The product builds plan 3 alone at N = 8192 and has no one-workgroup plan of N = 2^14, no one-launch form, no plans 8 / 12."""
    assert resolve(emu, 13, 9, 7, 0, 81)["plan"] == 3
    assert resolve(emu, 14, 43, 3, ROUND_ROBIN, 353, whole14_min=1, one_launch_min_tiles=1) == resolve(emu, 14, 43, 3, 0, 353)
    assert resolve(emu, 14, 43, 3, 0, 353)["whole"] == 0
    assert resolve(emu, 16, 11, 3, 0, 10337)["plan"] == 3 and resolve(emu, 16, 11, 3, 0, 18529)["plan"] == 3
