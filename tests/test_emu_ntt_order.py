"""The block order of the strided pass of a batched NTT launch pair (phantom-fhe_amd/csrc/pha_ntt_core.h: PassOrder), enumerated on
the CPU -- no GPU needed.  Harness: tests/emu/emu_ntt_order.cpp (test-only).  It builds the work maps of one launch with the
functions the launchers call (zloop_zper, zloop_fill, zloop_sub, pass_order_reverse) on the tile geometry of the real plans
(NttPlan<16, 10>, NttPlan<14, 3 / 4>, ...) and decodes every block of the grid with the function ntt_pass_kernel calls
(pass_order_decode), plus a margin of blocks past the grid's end.

Proved for every launch below:
  * the decode is a bijection from the grid's blocks onto the launch's (limb, polynomial, tile) set, and no block of the margin
    decodes to anything;
  * the limb sequence of the strided pass is exactly the reverse of the contiguous pass's limb list (ZloopMap: integer limbs first,
    then the FP64 limbs ascending), limb-major, with the polynomials descending inside a limb -- and, for the variant that keeps
    the integer limbs at the head, those first in the contiguous pass's order and the FP64 limbs reversed after them;
  * the two limb-range halves of a launch partition its limbs (ceil / floor), each with the same polynomials per workgroup and the
    same properties inside.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from util import MIXED_BITS, chain_bits

HERE = os.path.dirname(os.path.abspath(__file__))
MARGIN = 4099


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("emu_ntt_order") / "libemu_ntt_order.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fno-strict-aliasing", "-fPIC", "-shared", "-o", out,
                           os.path.join(HERE, "emu", "emu_ntt_order.cpp")])
    L = C.CDLL(out)
    L.emu_ntt_order.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32,
                                C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.emu_ntt_order.restype = C.c_int
    return L


def enumerate_launch(emu, log_n, variant, batch, bits, int_head=False, part=0, parts=1):
    """bits: prime sizes of the selected limbs.  None where the rule does not engage, else a dict of the harness's lists."""
    count = len(bits)
    fp = np.array([1 if b <= 50 else 0 for b in bits], dtype=np.uint8)
    cap = count * batch * 64 + MARGIN
    info = np.zeros(8, dtype=np.uint32)
    s_limbs = np.full(128, 255, dtype=np.uint8)
    dec = np.zeros((cap, 4), dtype=np.uint32)
    rc = emu.emu_ntt_order(log_n, variant, batch, count, fp.ctypes.data, int(int_head), part, parts, MARGIN, cap, info.ctypes.data,
                           s_limbs.ctypes.data, dec.ctypes.data)
    assert rc == 0, rc
    if info[0] == 0:
        return None
    blocks = int(info[3])
    return {"zper": int(info[0]), "lo": int(info[1]), "count": int(info[2]), "blocks": blocks, "tiles": int(info[4]),
            "zloop_blocks": int(info[5]), "n_int": int(info[6]), "s": [int(x) for x in s_limbs[:int(info[2])]],
            "dec": dec[:blocks + MARGIN].astype(np.int64), "fp": fp}


def prove(r, batch, int_head=False):
    blocks, tiles, count, lo = r["blocks"], r["tiles"], r["count"], r["lo"]
    limbs = list(range(lo, lo + count))
    s = r["s"]
    # the contiguous pass's list: a permutation of the part's limbs, the integer limbs first, each kind ascending
    assert sorted(s) == limbs
    ints, fps = s[:r["n_int"]], s[r["n_int"]:]
    assert all(not r["fp"][y] for y in ints) and all(r["fp"][y] for y in fps)
    assert ints == sorted(ints) and fps == sorted(fps)
    assert blocks == count * batch * tiles
    dec = r["dec"]
    inside, past = dec[:blocks], dec[blocks:]
    assert np.all(inside[:, 0] == 1), "a block of the grid decodes to nothing"
    assert np.all(past[:, 0] == 0), "a block past the grid decodes to work"
    y, z, t = inside[:, 1], inside[:, 2], inside[:, 3]
    assert y.min() >= lo and y.max() < lo + count and z.min() >= 0 and z.max() < batch and t.min() >= 0 and t.max() < tiles
    key = ((y - lo) * batch + z) * tiles + t
    assert np.array_equal(np.sort(key), np.arange(blocks)), "not a bijection onto (limb, polynomial, tile)"
    # limb-major: one run of batch x tiles blocks per limb; the runs in the reverse of S
    runs = y.reshape(count, batch * tiles)
    assert np.all(runs == runs[:, :1])
    want = ints + fps[::-1] if int_head else s[::-1]
    assert [int(v) for v in runs[:, 0]] == want
    # polynomials descending inside a limb, tiles inside a polynomial
    zz = z.reshape(count, batch, tiles)
    assert np.all(zz == np.arange(batch - 1, -1, -1)[None, :, None])
    assert np.all(t.reshape(count, batch, tiles) == np.arange(tiles)[None, None, :])


def _sel(total, start, count, pattern=MIXED_BITS):
    return chain_bits(total, pattern)[start:start + count]


# (id, log_n, plan, batch, prime sizes of the selection)
_LAUNCHES = [
    ("headline-16x45", 16, 10, 16, [60] + [50] * 44),                       # one integer limb at the head
    ("no-integer-limb", 16, 10, 8, [50, 48, 47, 46, 43, 42, 41, 40] * 2),
    ("integer-middle-and-end", 16, 10, 8, _sel(24, 0, 24)),                 # MIXED_BITS: limbs 3, 11, 15, 23
    ("integer-at-the-end-only", 16, 10, 8, [50] * 15 + [60]),
    ("several-integer-at-the-head", 16, 10, 8, [60, 55, 60] + [50] * 13),
    ("start-3-first-limb-integer", 16, 10, 8, _sel(20, 3, 16)),
    ("start-5", 16, 10, 16, _sel(40, 5, 33)),
    ("batch-8", 16, 10, 8, _sel(16, 0, 16)),
    ("batch-9-ragged", 16, 10, 9, _sel(16, 0, 16)),
    ("batch-11-ragged", 16, 10, 11, _sel(16, 0, 16)),
    ("batch-17", 16, 10, 17, _sel(32, 0, 32)),
    ("2^14-plan3-8x64", 14, 3, 8, _sel(64, 0, 64)),
    ("2^14-plan4-8x64", 14, 4, 8, _sel(64, 0, 64)),
    ("2^14-128-limbs-full-map", 14, 4, 8, [50, 48, 47, 46, 43, 42, 41, 40] * 8 + [61] * 64),
    ("2^15-plan4-8x32", 15, 4, 8, _sel(32, 0, 32)),
    ("2^17-plan4-8x8", 17, 4, 8, [50, 48, 47, 60, 46, 43, 42, 55]),
]


@pytest.mark.parametrize("int_head", [False, True], ids=["reverse", "integer-head"])
@pytest.mark.parametrize("case", _LAUNCHES, ids=[c[0] for c in _LAUNCHES])
def test_strided_order_is_a_bijection_in_the_reverse_of_the_contiguous_order(emu, case, int_head):
    _, log_n, variant, batch, bits = case
    r = enumerate_launch(emu, log_n, variant, batch, bits, int_head)
    assert r is not None, "the launcher rule should engage at this shape"
    assert r["lo"] == 0 and r["count"] == len(bits)
    prove(r, batch, int_head)


def test_polynomials_per_workgroup_follow_the_launcher_rule(emu):
    """zper as tests/test_gpu_ntt_plans.py reads it off launch_zloop: 8 x 16 limbs -> 4, 12 x 16 -> 3, 17 x 32 -> 6; the headline 16 x 45 -> 4
    (5760 wavefronts per polynomial x 2 groups < 12288)."""
    for batch, limbs, zper in [(8, 16, 4), (12, 16, 3), (17, 32, 6), (16, 45, 4)]:
        r = enumerate_launch(emu, 16, 10, batch, [50] * limbs)
        assert r["zper"] == zper
        assert r["zloop_blocks"] == limbs * 64 * -(-batch // zper)


@pytest.mark.parametrize("log_n,variant,batch,bits", [
    (16, 10, 8, [50] * 15),                                   # 128 x 15 x 2 = 3840 < 4096
    (16, 10, 7, [50] * 32),                                   # fewer than 8 polynomials
    (14, 3, 8, [50] * 63),                                    # 32 x 63 x 2 = 4032 < 4096
    (16, 10, 8, [50, 60, 47, 55, 42, 60, 36, 55, 50, 60, 47, 55, 42, 60, 60, 55]),   # 9 of 16 limbs on the integer back end
], ids=["8x15", "7x32", "2^14-8x63", "mostly-integer"])
def test_rule_does_not_engage(emu, log_n, variant, batch, bits):
    assert enumerate_launch(emu, log_n, variant, batch, bits) is None


@pytest.mark.parametrize("case", [
    ("odd-45", 16, 10, 16, [60] + [50] * 44),
    ("odd-mixed-33", 16, 10, 9, _sel(40, 5, 33)),
    ("even-16-integer-both-halves", 16, 10, 8, _sel(16, 0, 16)),
    ("2^14-128-limbs", 14, 4, 8, [50, 48, 47, 46, 43, 42, 41, 40] * 8 + [61] * 64),
    ("two-limbs", 16, 10, 64, [50, 48]),
], ids=lambda c: c[0])
@pytest.mark.parametrize("int_head", [False, True], ids=["reverse", "integer-head"])
def test_limb_range_halves(emu, case, int_head):
    """The halves of a launch: ceil(count / 2) limbs, then the rest; the whole launch decides zper."""
    _, log_n, variant, batch, bits = case
    whole = enumerate_launch(emu, log_n, variant, batch, bits, int_head)
    assert whole is not None
    halves = [enumerate_launch(emu, log_n, variant, batch, bits, int_head, part, 2) for part in (0, 1)]
    count = len(bits)
    assert [(h["lo"], h["count"]) for h in halves] == [(0, (count + 1) // 2), ((count + 1) // 2, count // 2)]
    for h in halves:
        assert h["zper"] == whole["zper"]
        prove(h, batch, int_head)
    # each half keeps the whole launch's order among its own limbs
    for h in halves:
        assert h["s"] == [y for y in whole["s"] if h["lo"] <= y < h["lo"] + h["count"]]
    assert sum(h["blocks"] for h in halves) == whole["blocks"]
    assert sum(h["zloop_blocks"] for h in halves) == whole["zloop_blocks"]


def test_one_limb_selection(emu):
    """One limb x 512 polynomials at N = 2^16 engages (128 x 1 x 64 groups); the strided pass is that limb, polynomials descending."""
    for bits in ([50], ):
        r = enumerate_launch(emu, 16, 10, 512, bits)
        assert r is not None and r["s"] == [0]
        prove(r, 512)
