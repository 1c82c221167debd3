"""Shared pieces of the BGV / BFV slot-semantics tests (tests/test_bv_semantics.py on the CPU, tests/test_gpu_bv_semantics.py on the
GPU), the twin of tests/ckks_semantics.py: what rotations, products, sums and matrix-vector products do to a BGV or BFV *message*,
compared with integers modulo t on the slots, where an answer is right or wrong with no tolerance.

* Messages are [N] integers modulo t = 65537, read as a 2 x N/2 matrix (rows(m)): the rotation by step s is np.roll(rows, -s, axis=1),
  Galois element 2N - 1 swaps the rows; products and sums are slot-wise modulo t (uint64: (t - 1)^2 * terms < 2^36).
* BvScheme: ckks_semantics.Scheme (secret key, s(X^g), key randomness) with what the two schemes add -- key noise scaled by t under
  BGV (generate_one_kswitch_key does that itself on the device; Scheme.oracle_key does not), encryption through
  encrypt_restatement.Restatement.symmetric with noise in [-21, 21], and a decryption of its own: the phase c0 + sum c_i s^i from
  oc.add / oc.multiply, the CRT in Python integers, then BGV: centre, reduce modulo t, times the inverse correction factor;
  BFV: round(t phase / Q) mod t.  Both return the margin in bits: BGV log2(Q_l / 2) - log2 max |centred phase|, BFV
  log2(0.5 / max distance of t phase / Q from an integer).
* CpuCodec / GpuCodec: slots -> plaintext by batch_restatement.Batch or by the library's BatchEncoder; decoding of a decrypted
  plaintext is always the restatement's.
* Reference: every operation of the cases composed from oracle steps (the CPU pipeline; its margin is the baseline of the GPU's).
* the case functions: the same inputs, seeds, expected slots and wrong answers for the oracle pipeline and the GPU pipeline.

MIN_MARGIN is a condition on the chosen inputs.  MARGIN_LOSS is ckks_semantics.FACTOR = 16 said in bits: the fused entries round once
where the composition rounds per step; a wrong constant costs tens of bits or every slot."""
import functools
import math

import numpy as np

import batch_restatement as B
from ckks_semantics import (Scheme, bsgs_diagonals, bsgs_diagonals_without_roll_back, elt_of_step,  # noqa: F401 (re-exported)
                            matrix_diagonals)
from encrypt_restatement import Restatement
from oracle import oracle as O

T = 65537
NOISE = 21
MIN_MARGIN = 8
MARGIN_LOSS = 4
TU = np.uint64(T)


def rows(m):
    """[..., N] -> [..., 2, N / 2]."""
    m = np.asarray(m)
    return m.reshape(m.shape[:-1] + (2, m.shape[-1] // 2))


def rot(m, step):
    """The rotation of both rows by `step`: slot i of a row takes slot i + step."""
    return np.roll(rows(m), -step, axis=-1).reshape(np.shape(m))


def swap(m):
    return rows(m)[..., ::-1, :].reshape(np.shape(m))


def messages(seed, count, n):
    return np.random.default_rng([0xB6F, seed]).integers(0, T, (count, n), dtype=np.uint64)


def matrix(seed, n_rows, n_cols):
    return np.random.default_rng([0xA7B, seed]).integers(0, T, (n_rows, n_cols), dtype=np.uint64)


def periodic(seed, d, n):
    """A random vector of period d in each row (the two rows differ), [N], and its two d-vectors [2][d]."""
    v = messages(seed, 1, 2 * d)[0].reshape(2, d)
    return np.tile(v, (1, n // 2 // d)).reshape(-1), v


def matvec(m, v):
    """m [r][d] times v [d] modulo t in Python integers."""
    return np.array([sum(int(a) * int(b) for a, b in zip(row, v)) % T for row in m], dtype=np.uint64)


def tiled(per_row, n):
    """[2][d] -> [N]: each row tiled over its N / 2 slots."""
    per_row = np.asarray(per_row)
    return np.tile(per_row, (1, n // 2 // per_row.shape[1])).reshape(-1)


def both_rows(diag):
    """A slot vector over N / 2 slots (what matrix_diagonals gives) -> [N], the same in both rows."""
    return np.concatenate([diag, diag], axis=-1)


def inv_t(f):
    return pow(int(f) % T, -1, T)


def differ(a, b):
    """The fraction of slots in which two slot arrays differ."""
    return float(np.mean(np.asarray(a) != np.asarray(b)))


# ---- key material, encryption, decryption -----------------------------------------------------------------------------------------
class BvScheme(Scheme):
    """One parameter set under BGV (NTT form) or BFV (coefficient form) with plain modulus T."""

    def __init__(self, name, kind, seed=1):
        super().__init__(name, seed)
        assert kind in (O.BGV, O.BFV) and (T - 1) % (2 * self.n) == 0
        self.kind = kind
        self.rest = Restatement(self.oc, kind, T)
        self.batch = B.batch(self.log_n, T)

    def tool(self, ql):
        if ql not in self._tools:
            self._tools[ql] = O.Tool(self.oc, ql).set_plain_modulus(T)
        return self._tools[ql]

    def oracle_key(self, elt=None):
        """Scheme.oracle_key with the noise scaled by t under BGV, before gen_kswitch_key."""
        if elt not in self._evk:
            new_key, a, e = self.relin_randomness() if elt is None else self.galois_randomness(elt)
            if self.kind == O.BGV:
                scalar = np.array([T % int(q) for q in self.primes], dtype=np.uint64)
                e = np.stack([self.oc.multiply_scalar(e[d], scalar, self.size_qp) for d in range(self.dnum)])
            e_ntt = np.stack([self._ntt(e[d], self.size_qp) for d in range(self.dnum)])
            self._evk[elt] = self.oc.gen_kswitch_key(self.sk_ntt, new_key, a, e_ntt)
        return self._evk[elt]

    def switch_factor(self, level):
        """The correction factor one mod_t_divide_q_last_ntt at `level` limbs multiplies in: q_last^-1 mod t."""
        return inv_t(self.primes[level - 1])

    def enc_randomness(self, level, tag):
        """(a [level][N] uniform, e [N] in [-NOISE, NOISE]) of the encryption named `tag`."""
        rng = self._rng("bv.enc", tag)
        return self._uniform(rng, self.primes[:level]), rng.integers(-NOISE, NOISE + 1, self.n)

    def encrypt(self, plain, level, tag):
        """plain [N] words below t -> [2][level][N] (BGV: NTT form, BFV: coefficient form)."""
        a, e = self.enc_randomness(level, tag)
        return self.rest.symmetric(self.sk_ntt, a, e, np.ascontiguousarray(plain, dtype=np.uint64), level)

    def phase(self, ct, level):
        """c0 + sum_i c_i s^i in coefficient form, [level][N]."""
        oc, s = self.oc, self.sk_ntt[:level]
        ct = np.ascontiguousarray(ct, dtype=np.uint64)
        ntt = ct if self.kind == O.BGV else np.stack([oc.nwt_forward(c, level, 0) for c in ct])
        acc, power = None, s
        for i in range(1, len(ct)):
            term = oc.multiply(ntt[i], power, level)
            acc = term if acc is None else oc.add(acc, term, level)
            power = oc.multiply(power, s, level)
        if self.kind == O.BGV:
            return oc.nwt_backward(oc.add(ntt[0], acc, level), level, 0)
        return oc.add(ct[0], oc.nwt_backward(acc, level, 0), level)

    def compose(self, coeff, level):
        """CRT in Python integers: [level][N] -> (object array [N] in [0, Q), Q)."""
        q = [int(p) for p in self.primes[:level]]
        big = math.prod(q)
        acc = np.zeros(self.n, dtype=object)
        for l, p in enumerate(q):
            mi = big // p
            acc = acc + coeff[l].astype(object) * (mi * pow(mi, -1, p) % big)
        return acc % big, big

    def decrypt(self, ct, level):
        """-> (plaintext [N] words below t BEFORE the correction factor, margin in bits)."""
        v, big = self.compose(self.phase(ct, level), level)
        if self.kind == O.BGV:
            centred = [int(x) - big if int(x) > big // 2 else int(x) for x in v]
            worst = max(abs(x) for x in centred)
            plain = np.array([x % T for x in centred], dtype=np.uint64)
        else:
            scaled = [int(x) * T for x in v]
            worst = max(min(x % big, big - x % big) for x in scaled)
            plain = np.array([((x + big // 2) // big) % T for x in scaled], dtype=np.uint64)
        margin = math.log2(big // 2) - (math.log2(worst) if worst else 0.0)
        return plain, margin

    def decode_ct(self, ct, level, factor=1):
        """Decrypt, apply the inverse correction factor, decode: (slots [N], margin)."""
        plain, margin = self.decrypt(ct, level)
        plain = plain * np.uint64(inv_t(factor)) % TU
        return self.batch.decode(plain), margin


@functools.lru_cache(maxsize=None)
def scheme(name, kind):
    return BvScheme(name, kind)


class CpuCodec:
    def __init__(self, sch):
        self.sch = sch

    def encode(self, values):
        """[count][N] slots -> [count][N] plaintext words below t."""
        return np.stack([self.sch.batch.encode(np.ascontiguousarray(v, dtype=np.uint64)) for v in np.atleast_2d(values)])


class GpuCodec:
    """The library's BatchEncoder behind the same call; the destination is poisoned first."""

    POISON = -0x2152411021524111

    def __init__(self, sch, P, enc, device):
        self.sch, self.P, self.enc, self.device = sch, P, enc, device

    def encode_device(self, values):
        import torch
        v = np.array(values, dtype=np.uint64, ndmin=2)
        dst = torch.full((v.shape[0], self.sch.n), self.POISON, dtype=torch.int64, device=self.device)
        self.enc.encode_batched(self.P.to_device(v, self.device), v.shape[1], dst)
        return dst

    def encode(self, values):
        return self.P.to_host(self.encode_device(values))


# ---- results ----------------------------------------------------------------------------------------------------------------------
class Result:
    """The ciphertexts one case produced, decrypted and decoded by the helper.  cts: list of [k][level][N]; want and every entry of
    wrongs: [len(cts)][N] slots; factor: the BGV correction factor the result carries (1 under BFV)."""

    def __init__(self, sch, label, cts, level, want, wrongs=(), factor=1):
        self.label, self.level, self.factor = label, level, int(factor)
        self.cts = [np.ascontiguousarray(c) for c in cts]
        self.want, self.wrongs = np.asarray(want, dtype=np.uint64), [np.asarray(w, dtype=np.uint64) for w in wrongs]
        assert self.want.shape == (len(self.cts), sch.n), label
        raw = [sch.decode_ct(ct, level) for ct in self.cts]
        self.raw = np.stack([r[0] for r in raw])                    # decoded with factor 1
        self.margin = min(r[1] for r in raw)
        self.got = self.raw * np.uint64(inv_t(factor)) % TU         # decoding is linear: the factor applies to the slots as well
        self.exact = bool(np.array_equal(self.got, self.want))
        self.bad_slots = int(np.count_nonzero(self.got != self.want))

    def factor_controls(self):
        """The result decoded with a missing, a doubled and an un-inverted correction factor (BGV results whose factor is not 1)."""
        if self.factor == 1:
            return []
        f = self.factor
        return [self.raw, self.raw * np.uint64(inv_t(f * f)) % TU, self.raw * np.uint64(f) % TU]


def check(res, floor=MIN_MARGIN):
    """Exact in all slots, margin >= floor, every wrong answer and every wrong factor off in more than half of the slots."""
    assert res.exact, f"{res.label}: {res.bad_slots} of {res.want.size} slots differ from the integers"
    assert res.margin >= floor, f"{res.label}: margin {res.margin:.1f} bits, floor {floor:.1f}"
    for i, w in enumerate(res.wrongs):
        assert differ(w, res.want) > 0.5, f"{res.label}: wrong answer {i} is too close to the right one"
    for i, w in enumerate(res.factor_controls()):
        assert differ(w, res.want) > 0.5, f"{res.label}: decoded with wrong factor {i} it still matches"


def _enc(sch, codec, z, level, tag):
    pts = codec.encode(z)
    return [sch.encrypt(pts[k], level, f"{tag}.{k}") for k in range(len(pts))]


# ---- the cases --------------------------------------------------------------------------------------------------------------------
def case_rotation(sch, codec, rotate_many, level, step, batch=1):
    """rotate_many(list of ct, level, elt) -> list of ct.  step None: the row swap (element 2N - 1)."""
    z = messages(11, batch, sch.n)
    cts = _enc(sch, codec, z, level, "rot")
    if step is None:
        out = rotate_many(cts, level, 2 * sch.n - 1)
        return Result(sch, "row swap", out, level, swap(z), [z, rot(z, 1), rot(swap(z), 1)])
    out = rotate_many(cts, level, elt_of_step(step, sch.n))
    wrongs = [z, swap(rot(z, step))] + ([rot(z, -step)] if (2 * step) % (sch.n // 2) else [])
    return Result(sch, f"rotate {step}", out, level, rot(z, step), wrongs)


def product_wrongs(z1, z2):
    return [z1, z2, (z1 + z2) % TU, z1 * swap(z2) % TU]


def case_products(sch, codec, multiply_many, level, batch, square=False, label="product"):
    """multiply_many(list of a, list of b, level) -> (list of size-2 ct, their level, their factor); square: b is a."""
    z = messages(12, 2 * batch, sch.n)
    a = _enc(sch, codec, z[:batch], level, "mul.a")
    b = a if square else _enc(sch, codec, z[batch:], level, "mul.b")
    z2 = z[:batch] if square else z[batch:]
    out, out_level, factor = multiply_many(a, b, level)
    wrongs = [z[:batch], (2 * z[:batch]) % TU, z[:batch] * swap(z[:batch]) % TU] if square else product_wrongs(z[:batch], z2)
    return Result(sch, label + (" (square)" if square else ""), out, out_level, z[:batch] * z2 % TU, wrongs, factor)


def case_inner_product(sch, codec, inner, level, terms, groups, shared):
    """inner(a [groups][terms] ct, b [groups][terms] or, shared, [terms], level) -> (list of [groups] ct, level, factor)."""
    za = messages(13, groups * terms, sch.n).reshape(groups, terms, -1)
    zb = messages(14, groups * terms, sch.n).reshape(groups, terms, -1)
    a = [_enc(sch, codec, za[g], level, f"ip.a{g}") for g in range(groups)]
    if shared:
        zb = np.broadcast_to(zb[0], zb.shape)
        b = _enc(sch, codec, zb[0], level, "ip.b0")
    else:
        b = [_enc(sch, codec, zb[g], level, f"ip.b{g}") for g in range(groups)]
    out, out_level, factor = inner(a, b, level)
    want = np.sum(za * zb % TU, axis=1) % TU
    wrongs = [(za * zb % TU)[:, 0], np.sum(za[::-1] * zb % TU, axis=1) % TU, np.sum(za * swap(zb) % TU, axis=1) % TU]
    return Result(sch, "inner product" + (" (operand 2 shared)" if shared else ""), out, out_level, want, wrongs, factor)


def case_plain_sum(sch, codec, plain_sum, level, terms, groups, with_acc):
    """plain_sum(plain [groups][terms][N] plaintext words, ct [groups][terms], acc [groups] or None, level) -> (cts, level, factor)."""
    zp = messages(15, groups * terms, sch.n).reshape(groups, terms, -1)
    zc = messages(16, groups * terms, sch.n).reshape(groups, terms, -1)
    zacc = messages(17, groups, sch.n)
    plain = np.stack([codec.encode(zp[g]) for g in range(groups)])
    ct = [_enc(sch, codec, zc[g], level, f"ps.c{g}") for g in range(groups)]
    acc = _enc(sch, codec, zacc, level, "ps.acc") if with_acc else None
    out, out_level, factor = plain_sum(plain, ct, acc, level)
    dot = np.sum(zp * zc % TU, axis=1) % TU
    want = (dot + zacc) % TU if with_acc else dot
    wrongs = [dot if with_acc else (dot + zacc) % TU, (zp * zc % TU)[:, 0], np.sum(zp * swap(zc) % TU, axis=1) % TU]
    return Result(sch, "plain sum" + (" + acc" if with_acc else ""), out, out_level, want, wrongs, factor)


def case_hoisting(sch, codec, hoist_many, level, steps, batch):
    """hoist_many(list of ct, level, elts) -> list of ct."""
    z = messages(18, batch, sch.n)
    cts = _enc(sch, codec, z, level, "hoist")
    out = hoist_many(cts, level, [elt_of_step(s, sch.n) for s in steps])
    want = sum(rot(z, s) for s in steps) % TU
    wrongs = [sum(rot(z, -s) for s in steps) % TU, len(steps) * z % TU, swap(want)]
    return Result(sch, f"hoisting {list(steps)}", out, level, want, wrongs)


def matvec_wrongs(m, v, n):
    """The transpose, a vector off by one slot either way, the rows swapped, the vector itself."""
    right = np.stack([matvec(m, v[r]) for r in range(2)])
    return [tiled(np.stack([matvec(m.T, v[r]) for r in range(2)]), n), tiled(np.stack([matvec(m, np.roll(v[r], 1)) for r in range(2)]), n),
            tiled(np.stack([matvec(m, np.roll(v[r], -1)) for r in range(2)]), n), tiled(right[::-1], n), tiled(v, n)]


def _matvec_want(m, tv, n):
    want = np.stack([tiled(np.stack([matvec(m, v[r]) for r in range(2)]), n) for _, v in tv])
    wrongs = [np.stack(w) for w in zip(*[matvec_wrongs(m, v, n) for _, v in tv])]
    return want, wrongs


def case_matvec(sch, codec, matvec_many, level, d, batch):
    """matvec_many(list of ct, level, diagonals [d][N] plaintext words, elts) -> list of ct at the same level, factor 1."""
    m = matrix(d, d, d)
    tv = [periodic(100 * d + b, d, sch.n) for b in range(batch)]
    cts = _enc(sch, codec, np.stack([t for t, _ in tv]), level, f"mv{d}")
    diags = codec.encode(both_rows(matrix_diagonals(m, sch.n // 2)))
    out = matvec_many(cts, level, diags, [elt_of_step(s, sch.n) for s in range(d)])
    want, wrongs = _matvec_want(m, tv, sch.n)
    return Result(sch, f"diag matvec {d} x {d}", out, level, want, wrongs)


def _bsgs_elts(sch, n_baby, n_giant):
    return [elt_of_step(j, sch.n) for j in range(n_baby)], [elt_of_step(i * n_baby, sch.n) for i in range(n_giant)]


def _bsgs_plain(codec, values):
    """[n_giant][n_baby] slot vectors over N / 2 slots -> the same nesting of plaintexts [N]."""
    flat = codec.encode(np.stack([both_rows(w) for row in values for w in row]))
    nb = len(values[0])
    return [[flat[i * nb + j] for j in range(nb)] for i in range(len(values))]


def bsgs_apply(weights, v, n_baby):
    """Integers: sum_i rotate_{i n_baby}(sum_j weights[i][j] o rotate_j(v)) on [N] slots, weights over N / 2 slots."""
    out = np.zeros_like(v)
    for i, row in enumerate(weights):
        inner = sum(both_rows(w) * rot(v, j) % TU for j, w in enumerate(row)) % TU
        out = (out + rot(inner, i * n_baby)) % TU
    return out


def case_bsgs(sch, codec, bsgs_many, level, n_baby, n_giant, batch, prepare=bsgs_diagonals):
    """bsgs_many(list of ct, level, baby elts, giant elts, weights [n_giant][n_baby] plaintexts [N]) -> list of ct, same level."""
    d = n_baby * n_giant
    m = matrix(1000 + d, d, d)
    tv = [periodic(200 * d + b, d, sch.n) for b in range(batch)]
    cts = _enc(sch, codec, np.stack([t for t, _ in tv]), level, f"bsgs{d}")
    baby, giant = _bsgs_elts(sch, n_baby, n_giant)
    out = bsgs_many(cts, level, baby, giant, _bsgs_plain(codec, prepare(m, sch.n // 2, n_baby, n_giant)))
    want, wrongs = _matvec_want(m, tv, sch.n)
    wrongs.append(np.stack([bsgs_apply(bsgs_diagonals_without_roll_back(m, sch.n // 2, n_baby, n_giant), t, n_baby) for t, _ in tv]))
    return Result(sch, f"bsgs matvec {n_baby} x {n_giant}", out, level, want, wrongs)


def case_bsgs_blocks(sch, codec, bsgs_blocks, level, n_baby, n_giant, n_blocks, prepare=bsgs_diagonals):
    """Row blocks of a (n_blocks d) x d matrix against one vector: bsgs_blocks(ct, level, baby, giant, [weights per block]) -> one
    ciphertext per block."""
    d = n_baby * n_giant
    m = matrix(2000 + d, n_blocks * d, d)
    t, v = periodic(300 * d, d, sch.n)
    ct = _enc(sch, codec, t[None], level, f"blocks{d}")[0]
    baby, giant = _bsgs_elts(sch, n_baby, n_giant)
    blocks = [m[r * d:(r + 1) * d] for r in range(n_blocks)]
    out = bsgs_blocks(ct, level, baby, giant, [_bsgs_plain(codec, prepare(blk, sch.n // 2, n_baby, n_giant)) for blk in blocks])
    want = np.stack([tiled(np.stack([matvec(blk, v[r]) for r in range(2)]), sch.n) for blk in blocks])
    wrongs = [np.stack(w) for w in zip(*[matvec_wrongs(blk, v, sch.n) for blk in blocks])]
    wrongs.append(want[::-1])
    return Result(sch, f"bsgs blocks {n_blocks} of {d} x {d}", out, level, want, wrongs)


def case_relin_rotate(sch, codec, relin_rotate_many, level, batch, step=1):
    """relin_rotate_many(list of a, list of b, level, elt) -> list of ct at the same level: the size-3 products, relinearised and
    rotated in one call."""
    z = messages(19, 2 * batch, sch.n)
    a = _enc(sch, codec, z[:batch], level, "rr.a")
    b = _enc(sch, codec, z[batch:], level, "rr.b")
    out = relin_rotate_many(a, b, level, elt_of_step(step, sch.n))
    zz = z[:batch] * z[batch:] % TU
    return Result(sch, f"relinearize + rotate {step}", out, level, rot(zz, step), [rot(zz, -step), zz, swap(rot(zz, step)), rot(z[:batch], step)])


def case_depth_two(sch, codec, multiply_many, bring_down, level):
    """(a b) c: multiply_many as in case_products; bring_down(ct, level) -> (ct, level, factor) takes a fresh ciphertext to the level
    of the first product (BGV: one modulus switch; BFV: None, the level does not change)."""
    z = messages(21, 3, sch.n)
    a, b, c = _enc(sch, codec, z, level, "d2")
    (ab,), l1, f1 = multiply_many([a], [b], level)
    c, lc, fc = bring_down(c, level) if bring_down else (c, level, 1)
    assert lc == l1
    (out,), l2, f2 = multiply_many([ab], [c], l1)
    want = (z[0] * z[1] % TU * z[2] % TU)[None]
    factor = f1 * fc % T * f2 % T
    return Result(sch, "depth two", [out], l2, want, [(z[0] * z[1] % TU)[None], (z[0] * z[2] % TU)[None], swap(want)], factor)


def case_bfv_plain_ops(sch, codec, api, level):
    """BFV on plaintexts [N] below t: api.plain_sum(plain [groups][terms][N], ct [groups][terms], acc [groups], level), api.add_plain(ct,
    plain, level, subtract), api.multiply_plain(ct, plain, level) -> ciphertexts in coefficient form."""
    terms, groups, n = 3, 2, sch.n
    zp = messages(31, groups * terms, n).reshape(groups, terms, -1)
    zc = messages(32, groups * terms, n).reshape(groups, terms, -1)
    zacc = messages(33, groups, n)
    plain = np.stack([codec.encode(zp[g]) for g in range(groups)])
    ct = [_enc(sch, codec, zc[g], level, f"bp.c{g}") for g in range(groups)]
    acc = _enc(sch, codec, zacc, level, "bp.acc")
    dot = np.sum(zp * zc % TU, axis=1) % TU
    out = [Result(sch, "bfv plain sum + acc", api.plain_sum(plain, ct, acc, level), level, (dot + zacc) % TU,
                  [dot, (zp * zc % TU)[:, 0], np.sum(zp * swap(zc) % TU, axis=1) % TU])]
    x, p, zx, zq = ct[0][0], plain[0][1], zc[0, 0], zp[0, 1]
    out.append(Result(sch, "bfv add_plain", [api.add_plain(x, p, level, False)], level, ((zx + zq) % TU)[None], [zx[None], ((zx + TU - zq) % TU)[None]]))
    out.append(Result(sch, "bfv sub_plain", [api.add_plain(x, p, level, True)], level, ((zx + TU - zq) % TU)[None], [zx[None], ((zx + zq) % TU)[None]]))
    out.append(Result(sch, "bfv multiply_plain", [api.multiply_plain(x, p, level)], level, (zx * zq % TU)[None],
                      [w[None] for w in product_wrongs(zx, zq)]))
    return out


# ---- the evaluator level (host/phantom.h through pyPhantom on the GPU) -----------------------------------------------------------------
HOST_STEPS = (1, 2, 5)


def balance(f1, f2):
    """balance_correction_factors as the reference states it (src/evaluate.cu:20-77), in Python integers: along the extended Euclidean
    remainder sequence a = b f2 / f1 (mod t) of (t, f2 / f1), the pair (e1, e2) = (a, b) of smallest |e1| + |e2| (centred).
    -> (common factor e1 f1, e1, e2), e1 and e2 as residues in [0, t): that is how add_inplace multiplies them into the ciphertexts, so
    a negative e costs log2 t bits of noise where its centred value would cost log2 |e| (balance_centred has those)."""
    centred = lambda x: x - T if x > T // 2 else x
    ratio = int(f2) * inv_t(f1) % T
    e1, e2 = ratio, 1
    best = abs(centred(e1)) + abs(centred(e2))
    prev_a, prev_b, a, b = T, 0, ratio, 1
    while a:
        q = prev_a // a
        prev_a, a = a, prev_a % a
        prev_b, b = b, prev_b - b * q
        if a % T and math.gcd(a % T, T) == 1 and abs(centred(a % T)) + abs(centred(b % T)) < best:
            e1, e2 = a % T, b % T
            best = abs(centred(e1)) + abs(centred(e2))
    return e1 * int(f1) % T, e1, e2


def balance_centred(f1, f2):
    """The pair of smallest |e1| + |e2| by exhaustion over e2, centred: what the sum could cost at best."""
    e2 = np.arange(1, T, dtype=np.int64)
    e1 = e2 * (int(f2) * inv_t(f1) % T) % T
    c1, c2 = np.where(e1 > T // 2, e1 - T, e1), np.where(e2 > T // 2, e2 - T, e2)
    k = int(np.argmin(np.abs(c1) + np.abs(c2)))
    return int(e1[k]) * int(f1) % T, int(c1[k]), int(c2[k])


def case_host_bgv(sch, codec, api):
    """A ciphertext is (numpy [2][limbs][N], limbs, correction factor) on both sides of `api`; every reported factor must be the one
    that makes the helper's decryption exact.  api: multiply_relin_mod_switch(x, y), multiply_relinearize_switch(x, y) (three
    calls), mod_switch(x), rotate(x, step), hoisting(x, steps), add(x, y), sub(x, y), add_plain(x, plain [N]), multiply_plain(x, plain),
    add_many([x, ...])."""
    top, n = sch.size_q, sch.n
    z = messages(41, 5, n)
    a, b, c, d = [(ct, top, 1) for ct in _enc(sch, codec, z[:4], top, "host")]
    pt = codec.encode(z[4:])[0]
    out = []

    def check(label, res, want, wrongs, limbs, factor=None):
        ct, got_limbs, got_factor = res
        assert got_limbs == limbs and ct.shape == (2, limbs, n), f"{label}: {got_limbs} limbs, want {limbs}"
        assert factor is None or got_factor == factor, f"{label}: correction factor {got_factor}, want {factor}"
        out.append(Result(sch, label, [ct], limbs, want[None], [w[None] for w in wrongs], got_factor))
        return res

    mul = lambda x, y: x * y % TU
    f5, f4 = sch.switch_factor(top), sch.switch_factor(top - 1)
    ab = check("multiply_relin_mod_switch", api.multiply_relin_mod_switch(a, b), mul(z[0], z[1]), product_wrongs(z[0], z[1]), top - 1, f5)
    cd = api.multiply_relin_mod_switch(c, d)
    abcd = check("multiply_relin_mod_switch twice", api.multiply_relin_mod_switch(ab, cd), mul(mul(z[0], z[1]), mul(z[2], z[3])),
                 [mul(z[0], z[1]), mul(z[2], z[3])], top - 2, f5 * f5 * f4 % T)
    check("multiply + relinearize + mod_switch_to_next", api.multiply_relinearize_switch(a, b), mul(z[0], z[1]), product_wrongs(z[0], z[1]),
          top - 1, f5)
    check("rotate 1", api.rotate(a, 1), rot(z[0], 1), [rot(z[0], -1), z[0], swap(rot(z[0], 1))], top, 1)
    check("rotate 2 of a product", api.rotate(ab, 2), rot(mul(z[0], z[1]), 2), [rot(mul(z[0], z[1]), -2), mul(z[0], z[1])], top - 1, f5)
    check("hoisting [1, 2, 5]", api.hoisting(a, list(HOST_STEPS)), sum(rot(z[0], s) for s in HOST_STEPS) % TU,
          [sum(rot(z[0], -s) for s in HOST_STEPS) % TU, 3 * z[0] % TU], top, 1)
    a4 = check("mod_switch_to_next twice", api.mod_switch(api.mod_switch(a)), z[0], [swap(z[0])], top - 2, f5 * f4 % T)
    assert a4[2] != abcd[2]
    zs = mul(mul(z[0], z[1]), mul(z[2], z[3]))
    check("add (different factors)", api.add(abcd, a4), (zs + z[0]) % TU, [zs, z[0], (zs + TU - z[0]) % TU], top - 2)
    check("sub (different factors)", api.sub(abcd, a4), (zs + TU - z[0]) % TU, [zs, (zs + z[0]) % TU, (z[0] + TU - zs) % TU], top - 2)
    check("add_many (different factors)", api.add_many([a4, abcd, a4]), (zs + 2 * z[0]) % TU, [zs, (zs + z[0]) % TU], top - 2)
    check("add_plain (factor not 1)", api.add_plain(ab, pt), (mul(z[0], z[1]) + z[4]) % TU,
          [mul(z[0], z[1]), (mul(z[0], z[1]) + mul(z[4], np.uint64(inv_t(f5)))) % TU], top - 1, f5)
    check("multiply_plain (factor not 1)", api.multiply_plain(ab, pt), mul(mul(z[0], z[1]), z[4]), [mul(z[0], z[1]), mul(z[0], z[4])], top - 1, f5)
    return out


def case_host_bfv(sch, codec, api):
    """api: multiply_and_relin(x, y), rotate(x, step), add_plain(x, plain, subtract), multiply_plain(x, plain), add_many([x, ...]) on
    numpy ciphertexts [2][Q][N] in coefficient form."""
    top, n = sch.size_q, sch.n
    z = messages(42, 4, n)
    a, b, c = _enc(sch, codec, z[:3], top, "host")
    pt = codec.encode(z[3:])[0]
    mul = lambda x, y: x * y % TU
    one = lambda label, ct, want, wrongs: Result(sch, label, [ct], top, want[None], [w[None] for w in wrongs])
    return [one("multiply_and_relin", api.multiply_and_relin(a, b), mul(z[0], z[1]), product_wrongs(z[0], z[1])),
            one("rotate 1", api.rotate(a, 1), rot(z[0], 1), [rot(z[0], -1), z[0], swap(rot(z[0], 1))]),
            one("rotate 5", api.rotate(a, 5), rot(z[0], 5), [rot(z[0], -5), z[0]]),
            one("add_plain", api.add_plain(a, pt, False), (z[0] + z[3]) % TU, [z[0], (z[0] + TU - z[3]) % TU]),
            one("sub_plain", api.add_plain(a, pt, True), (z[0] + TU - z[3]) % TU, [z[0], (z[0] + z[3]) % TU]),
            one("multiply_plain", api.multiply_plain(a, pt), mul(z[0], z[3]), product_wrongs(z[0], z[3])),
            one("add_many", api.add_many([a, b, c]), (z[0] + z[1] + z[2]) % TU, [(z[0] + z[1]) % TU, z[0]])]


# ---- the oracle pipeline ------------------------------------------------------------------------------------------------------------
class Reference:
    """The operations of the cases composed from oracle steps on numpy ciphertexts."""

    def __init__(self, sch):
        self.sch, self.oc, self.kind = sch, sch.oc, sch.kind
        self._mul = {}

    def add_ct(self, a, b, level):
        return np.stack([self.oc.add(a[p], b[p], level) for p in range(len(a))])

    def galois(self, poly, level, elt):
        if self.kind == O.BFV:
            return self.oc.apply_galois_coeff(poly, int(elt), level)
        return O.apply_galois_ntt(poly, O.galois_ntt_table(self.sch.log_n, int(elt)), self.sch.n, level)

    def rotate(self, ct, level, elt):
        c0, c1 = (self.galois(ct[p], level, elt) for p in range(2))
        return self.sch.tool(level).keyswitch_inplace(np.stack([c0, np.zeros_like(c0)]), c1, self.sch.digits(int(elt), level), self.kind)

    def rotate_many(self, cts, level, elt):
        return [self.rotate(ct, level, elt) for ct in cts]

    def relinearize(self, ct3, level):
        return self.sch.tool(level).keyswitch_inplace(ct3[:2], ct3[2], self.sch.digits(None, level), self.kind)

    def mod_switch(self, ct, level):
        """-> (ct at level - 1, level - 1, the factor the switch multiplies in)."""
        return self.sch.tool(level).mod_t_divide_q_last_ntt(ct, len(ct)), level - 1, self.sch.switch_factor(level)

    def tensor(self, x, y, level):
        return self.oc.tensor_square_2x2(x, level) if y is x else self.oc.tensor_prod_2x2(x, y, level)

    # -- BGV ----------------------------------------------------------------------------------------------------------------------
    def bgv_multiply_many(self, a, b, level):
        out = [self.mod_switch(self.relinearize(self.tensor(x, y, level), level), level)[0] for x, y in zip(a, b)]
        return out, level - 1, self.sch.switch_factor(level)

    def _summed(self, a, b, level):
        out = []
        for g, row in enumerate(a):
            other, t3 = (b[g] if isinstance(b[0], list) else b), None
            for x, y in zip(row, other):
                t = self.oc.tensor_prod_2x2(x, y, level)
                t3 = t if t3 is None else self.add_ct(t3, t, level)
            out.append(self.relinearize(t3, level))
        return out

    def bgv_inner(self, a, b, level):
        return self._summed(a, b, level), level, 1

    def bgv_inner_switch(self, a, b, level):
        return [self.mod_switch(ct, level)[0] for ct in self._summed(a, b, level)], level - 1, self.sch.switch_factor(level)

    def bgv_plain_sum(self, plain, ct, acc, level):
        out = []
        for g in range(len(ct)):
            total = None if acc is None else acc[g]
            for p, c in zip(plain[g], ct[g]):
                w = self.oc.bgv_lift_plain(p, level)
                t = np.stack([self.oc.multiply(c[i], w, level) for i in range(2)])
                total = t if total is None else self.add_ct(total, t, level)
            out.append(self.mod_switch(total, level)[0])
        return out, level - 1, self.sch.switch_factor(level)

    def lift_wide(self, plain, level):
        """A plaintext [N] below t over the rows [0, level) u P in NTT form (every residue is the word itself: t is below every prime)."""
        rws = self.sch.rows(level, True)
        return self.oc.nwt_forward_map(np.tile(np.ascontiguousarray(plain, dtype=np.uint64), (len(rws), 1)), rws)

    def _keys(self, elts, level):
        return [None if e == 1 else self.sch.digits(e, level) for e in elts]

    def hoist_many(self, cts, level, elts):
        tool = self.sch.tool(level)
        return [tool.hoisting(ct, elts, [self.sch.digits(e, level) for e in elts], self.kind) for ct in cts]

    def matvec_many(self, cts, level, diags, elts):
        tool, ws = self.sch.tool(level), [self.lift_wide(p, level) for p in diags]
        return [tool.hoisting_weighted(ct, elts, self._keys(elts, level), ws, self.kind) for ct in cts]

    def bsgs_many(self, cts, level, baby, giant, weights):
        tool, ws = self.sch.tool(level), [[self.lift_wide(p, level) for p in row] for row in weights]
        return [tool.hoisting_weighted_bsgs(ct, baby, self._keys(baby, level), giant, self._keys(giant, level), ws, self.kind) for ct in cts]

    def bsgs_blocks(self, ct, level, baby, giant, blocks):
        return [self.bsgs_many([ct], level, baby, giant, weights)[0] for weights in blocks]

    def bgv_relin_rotate_many(self, a, b, level, elt):
        return [self.rotate(self.relinearize(self.oc.tensor_prod_2x2(x, y, level), level), level, elt) for x, y in zip(a, b)]

    # -- BFV ----------------------------------------------------------------------------------------------------------------------
    def multiplier(self, tech, size_ql=None):
        key = (tech, size_ql)
        if key not in self._mul:
            self._mul[key] = {"behz": O.Behz, "hps": O.Hps, "overq": O.HpsOverQ}[tech](self.oc, T, *([size_ql] if size_ql else []))
        return self._mul[key]

    def bfv_multiply_many(self, tech):
        """multiply_many of case_products: the `tech` product, then keyswitch_inplace at the top level.  Equal operands are two
        buffers with equal words (the same-pointer shortcut of hps_overq is not what the cases test)."""
        def run(a, b, level):
            mul = self.multiplier(tech)
            return [self.relinearize(mul.multiply(x, np.array(y, copy=True)), level) for x, y in zip(a, b)], level, 1
        return run

    def bfv_multiply_leveled(self, size_ql, fused):
        """hps_overq_leveled with size_Q - size_ql levels dropped: the product and the leveled key switch, or the fused entry."""
        def run(a, b, level):
            hq, tool = self.multiplier("overq", size_ql), self.sch.tool(size_ql)
            keys = self.sch.digits(None, size_ql)
            out = []
            for x, y in zip(a, b):
                y = np.array(y, copy=True)
                if fused:
                    out.append(hq.mul_relin_leveled(tool, x, y, keys))
                else:
                    p = hq.multiply(x, y)
                    out.append(hq.keyswitch_leveled(tool, p[:2], p[2], keys))
            return out, level, 1
        return run

    def bfv_relin_rotate_many(self, a, b, level, elt):
        mul = self.multiplier("behz")
        return [self.rotate(self.relinearize(mul.multiply(x, y), level), level, elt) for x, y in zip(a, b)]

    # BFV plaintext operations (case_bfv_plain_ops)
    def plain_sum(self, plain, ct, acc, level):
        out = []
        for g in range(len(ct)):
            total = acc[g]
            for p, c in zip(plain[g], ct[g]):
                total = self.add_ct(total, self.oc.bfv_multiply_plain(c, p, T), level)
            out.append(total)
        return out

    def add_plain(self, ct, plain, level, subtract):
        return np.stack([self.oc.bfv_add_plain(ct[0], plain, T, subtract), ct[1]])

    def multiply_plain(self, ct, plain, level):
        return self.oc.bfv_multiply_plain(ct, plain, T)


class ReferenceHostBgv:
    """case_host_bgv's `api` from oracle steps, with the correction-factor rules as the helper states them: a product multiplies the
    factors, a modulus switch multiplies by q_last^-1, a sum first brings both operands to a common factor (balance; centred: with
    balance_centred's scalars, what the reference does not do), add_plain adds factor * plain, multiply_plain leaves the factor."""

    def __init__(self, ref, centred=False):
        self.ref, self.sch, self.oc = ref, ref.sch, ref.sch.oc
        self.balance = balance_centred if centred else balance

    def _scaled(self, ct, e, limbs):
        scalar = np.array([e % int(q) for q in self.sch.primes[:limbs]], dtype=np.uint64)
        return np.stack([self.oc.multiply_scalar(ct[p], scalar, limbs) for p in range(len(ct))])

    def mod_switch(self, x):
        ct, limbs, f = x
        out, low, g = self.ref.mod_switch(ct, limbs)
        return out, low, f * g % T

    def multiply_relinearize_switch(self, x, y):
        (a, limbs, f1), (b, _, f2) = x, y
        return self.mod_switch((self.ref.relinearize(self.oc.tensor_prod_2x2(a, b, limbs), limbs), limbs, f1 * f2 % T))

    multiply_relin_mod_switch = multiply_relinearize_switch

    def rotate(self, x, step):
        return self.ref.rotate(x[0], x[1], elt_of_step(step, self.sch.n)), x[1], x[2]

    def hoisting(self, x, steps):
        return self.ref.hoist_many([x[0]], x[1], [elt_of_step(s, self.sch.n) for s in steps])[0], x[1], x[2]

    def _balanced(self, x, y):
        (a, limbs, f1), (b, _, f2) = x, y
        if f1 == f2:
            return a, b, limbs, f1
        common, e1, e2 = self.balance(f1, f2)
        return self._scaled(a, e1, limbs), self._scaled(b, e2, limbs), limbs, common

    def add(self, x, y):
        a, b, limbs, f = self._balanced(x, y)
        return self.ref.add_ct(a, b, limbs), limbs, f

    def sub(self, x, y):
        a, b, limbs, f = self._balanced(x, y)
        return np.stack([self.oc.sub(a[p], b[p], limbs) for p in range(2)]), limbs, f

    def add_many(self, xs):
        total = xs[0]
        for x in xs[1:]:
            total = self.add(total, x)
        return total

    def add_plain(self, x, plain):
        ct, limbs, f = x
        lifted = self._scaled(self.oc.bgv_lift_plain(plain, limbs)[None], f, limbs)[0]
        return np.stack([self.oc.add(ct[0], lifted, limbs), ct[1]]), limbs, f

    def multiply_plain(self, x, plain):
        ct, limbs, f = x
        lifted = self.oc.bgv_lift_plain(plain, limbs)
        return np.stack([self.oc.multiply(ct[p], lifted, limbs) for p in range(2)]), limbs, f


class ReferenceHostBfv:
    """case_host_bfv's `api` from oracle steps; tech: the multiply the context is set to."""

    def __init__(self, ref, tech):
        self.ref, self.sch, self.tech = ref, ref.sch, tech

    def multiply_and_relin(self, a, b):
        return self.ref.bfv_multiply_many(self.tech)([a], [b], self.sch.size_q)[0][0]

    def rotate(self, a, step):
        return self.ref.rotate(a, self.sch.size_q, elt_of_step(step, self.sch.n))

    def add_plain(self, a, plain, subtract):
        return self.ref.add_plain(a, plain, self.sch.size_q, subtract)

    def multiply_plain(self, a, plain):
        return self.ref.multiply_plain(a, plain, self.sch.size_q)

    def add_many(self, cts):
        total = cts[0]
        for ct in cts[1:]:
            total = self.ref.add_ct(total, ct, self.sch.size_q)
        return total


@functools.lru_cache(maxsize=None)
def cpu_host(name, kind, tech=None, centred=False):
    """The oracle pipeline of the evaluator-level case."""
    sch = scheme(name, kind)
    ref = Reference(sch)
    if kind == O.BGV:
        return case_host_bgv(sch, CpuCodec(sch), ReferenceHostBgv(ref, centred))
    return case_host_bfv(sch, CpuCodec(sch), ReferenceHostBfv(ref, tech))


# ---- the case list: one entry per (parameter set, scheme, case, oracle implementation, arguments) ------------------------------------
def _resolve(ref, spec):
    """An implementation of the oracle pipeline by name: "method", or ("factory", arguments...) for the ones that take a variant."""
    if spec is None or spec == "self":
        return ref if spec else None
    return getattr(ref, spec) if isinstance(spec, str) else getattr(ref, spec[0])(*spec[1:])


@functools.lru_cache(maxsize=None)
def cpu(name, kind, case, impls, *args):
    """The oracle pipeline of one case, computed once per process: its margin is the baseline of the GPU margin of the same case."""
    sch = scheme(name, kind)
    ref = Reference(sch)
    impls = impls if isinstance(impls, tuple) and impls and impls[0] == "+" else ("+", impls)
    return globals()["case_" + case](sch, CpuCodec(sch), *[_resolve(ref, s) for s in impls[1:]], *args)


BGV12, BGV14, BFV12, BFV13 = ("hyb12_a2", O.BGV), ("hyb14_a2", O.BGV), ("c1_bfv4096", O.BFV), ("bfv13_50", O.BFV)
