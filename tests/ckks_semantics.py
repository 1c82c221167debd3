"""Shared pieces of the CKKS slot-semantics tests (tests/test_ckks_semantics.py on the CPU, tests/test_gpu_ckks_semantics.py on the GPU):
what rotations, products and matrix-vector products do to a CKKS *message*, compared with numpy on the slot vectors.

* Scheme: key material and encryption on the CPU through the oracle, independent of the code under test -- a ternary secret, noise in
  [-3, 3], every draw from a generator seeded by (seed, purpose), so that the CPU and the GPU pipeline of one case see the same
  ciphertexts and the same key randomness; s(X^elt) from plain index arithmetic.
* CpuCodec / GpuCodec: message -> plaintext and plaintext -> message, by the numpy restatement (tests/ckks_restatement.py) or by
  the library's CKKSEncoder; numpy arrays in and out on both.
* Reference: every operation of the tests composed from oracle steps (the CPU pipeline; the baseline of the GPU bounds).
* bsgs_diagonals, nearest_wrong, bound: the preparation the diag_matvec_bsgs docstring describes, the negative controls, and the
  bound of a GPU error from the CPU error of the same case."""
import functools

import numpy as np

import ckks_restatement as R
from oracle import oracle as O
from util import oracle_ctx, primes_of

CAP = 2.0 ** -12            # no GPU error may exceed this, whatever the CPU error
CPU_CAP = 2.0 ** -16        # the oracle pipeline alone stays below this in every case
FACTOR = 16.0               # gpu_err <= FACTOR * cpu_err: fused entries round once where the composition rounds per step, key noise
                            # differs from draw to draw -- small factors; a wrong convention is 10^5 times the baseline or more
FAR = 0.1                   # every plausible wrong answer is farther than this from what was computed


def bound(cpu_err):
    return min(FACTOR * cpu_err, CAP)


def max_err(got, want):
    return float(np.max(np.abs(np.asarray(got) - np.asarray(want))))


def nearest_wrong(got, want_variants):
    """The smallest distance (max over the slots) from `got` to any of the plausible wrong answers."""
    return min(max_err(got, w) for w in want_variants)


def messages(seed, count, slots):
    """`count` random complex slot vectors with |re|, |im| <= 1."""
    rng = np.random.default_rng([0xC0FFEE, seed])
    return rng.uniform(-1, 1, (count, slots)) + 1j * rng.uniform(-1, 1, (count, slots))


def matrix(seed, rows, cols):
    """A random complex matrix, not symmetric, entries scaled so that |(M v)[i]| stays of order 1 for |v[i]| <= sqrt 2."""
    rng = np.random.default_rng([0xA7A7, seed])
    return (rng.uniform(-1, 1, (rows, cols)) + 1j * rng.uniform(-1, 1, (rows, cols))) / np.sqrt(cols)


def periodic(seed, d, slots):
    """A random complex vector of period d in the slots, and its d distinct values."""
    v = messages(seed, 1, d)[0]
    return np.tile(v, slots // d), v


def matrix_diagonals(m, slots, steps=None):
    """The test's own statement of the generalised diagonals: diag_k[i] = M[i % d][(i + k) % d]."""
    d = m.shape[0]
    i = np.arange(slots)
    return np.stack([m[i % d, (i + s) % d] for s in (range(d) if steps is None else steps)])


def bsgs_diagonals(m, slots, n_baby, n_giant):
    """out[i][j] = diagonal i * n_baby + j of m, rotated back by giant step i: np.roll(diag, +i * n_baby) (rotate_{-g}(d)[k] = d[k - g]),
    so that sum_i rotate_{i n_baby}(sum_j out[i][j] o rotate_j(v)) = m v.  Pins the sentence in workloads.diag_matvec_bsgs."""
    diags = matrix_diagonals(m, slots)
    assert n_baby * n_giant == m.shape[0]
    return [[np.roll(diags[i * n_baby + j], i * n_baby) for j in range(n_baby)] for i in range(n_giant)]


def bsgs_diagonals_without_roll_back(m, slots, n_baby, n_giant):
    """The wrong preparation (negative control): the diagonals as they are."""
    diags = matrix_diagonals(m, slots)
    return [[diags[i * n_baby + j] for j in range(n_baby)] for i in range(n_giant)]


def bsgs_apply(weights, v, n_baby):
    """numpy: sum_i rotate_{i n_baby}(sum_j weights[i][j] o rotate_j(v)), rotate_s(v) = np.roll(v, -s)."""
    out = np.zeros_like(v)
    for i, row in enumerate(weights):
        out = out + np.roll(sum(w * np.roll(v, -j) for j, w in enumerate(row)), -i * n_baby)
    return out


def elt_of_step(step, n):
    """Galois element of rotation step `step` (any integer; rotate_s(v)[i] = v[i + s]): 5^(s mod slots) mod 2N."""
    return int(pow(5, step % (n // 2), 2 * n))


def rotation_wrongs(z, step):
    """Plausible wrong answers of a rotation by `step`: the opposite direction (unless it is the same vector: 2 s = 0 mod slots),
    the conjugate, the conjugate of the right answer, the unrotated message."""
    out = [np.conj(z), np.conj(np.roll(z, -step)), z]
    if (2 * step) % len(z):
        out.append(np.roll(z, step))
    return out


def product_wrongs(z1, z2):
    return [z1, z2, z1 * np.conj(z2), np.conj(z1 * z2), z1 + z2]


def matvec_wrongs(m, v, slots):
    """Plausible wrong answers of a square matrix-vector product: the transpose, conjugates, a vector off by one slot, the vector."""
    d = m.shape[0]
    return [np.tile(x, slots // d) for x in (m.T @ v, np.conj(m) @ v, np.conj(m @ v), m @ np.roll(v, 1), m @ np.roll(v, -1), v)]


class Scheme:
    """One parameter set with a secret key; ciphertexts are numpy [size][Ql][N] in NTT form, limbs [0, Ql)."""

    def __init__(self, name, seed=1):
        self.name, self.seed = name, seed
        self.log_n, self.primes, self.size_p = primes_of(name)
        self.n = 1 << self.log_n
        self.slots = self.n // 2
        self.size_qp = len(self.primes)
        self.size_q = self.size_qp - self.size_p
        self.dnum = self.size_q // self.size_p
        self.oc = oracle_ctx(name)
        self.s_small = self._rng("sk").integers(-1, 2, self.n)
        self.sk_ntt = self._ntt(self._residues(self.s_small, self.primes), self.size_qp)
        self._tools, self._evk = {}, {}

    def _rng(self, *tag):
        return np.random.default_rng([self.seed] + [int.from_bytes(str(t).encode(), "little") % (1 << 63) for t in tag])

    @staticmethod
    def _residues(small, primes):
        small = np.asarray(small, dtype=np.int64)
        return np.stack([np.mod(small, np.int64(int(q))).astype(np.uint64) for q in primes])

    def _ntt(self, x, limbs):
        return self.oc.nwt_forward(x, limbs, 0)

    def _uniform(self, rng, primes):
        return np.stack([rng.integers(0, int(q), self.n, dtype=np.uint64) for q in primes])

    def tool(self, ql):
        if ql not in self._tools:
            self._tools[ql] = O.Tool(self.oc, ql)
        return self._tools[ql]

    def rows(self, ql, with_special):
        return list(range(ql)) + (list(range(self.size_q, self.size_qp)) if with_special else [])

    # -- the secret key under an automorphism ----------------------------------------------------------------------------------------
    def sk_galois_ntt(self, elt):
        """s(X^elt) over QP in NTT form: coefficient i goes to i * elt mod 2N, negated past N."""
        at = (np.arange(self.n, dtype=np.int64) * int(elt)) % (2 * self.n)
        out = np.zeros(self.n, dtype=np.int64)
        out[at % self.n] = np.where(at >= self.n, -self.s_small, self.s_small)
        return self._ntt(self._residues(out, self.primes), self.size_qp)

    # -- encryption --------------------------------------------------------------------------------------------------------------------
    def encrypt(self, pt_ntt, level, tag=0):
        """(c0, c1) with c0 + c1 s = pt + e; pt_ntt [level][N]; the draws depend on (seed, tag) only."""
        rng, q = self._rng("enc", tag), self.primes[:level]
        c1 = self._uniform(rng, q)
        e = self._ntt(self._residues(rng.integers(-3, 4, self.n), q), level)
        oc = self.oc
        c0 = oc.sub(oc.add(np.ascontiguousarray(pt_ntt[:level]), e, level), oc.multiply(c1, self.sk_ntt[:level], level), level)
        return np.stack([c0, c1])

    def decrypt(self, ct, level):
        """c0 + c1 s (+ c2 s^2), NTT form [level][N]."""
        oc, s = self.oc, self.sk_ntt[:level]
        out = oc.add(ct[0], oc.multiply(ct[1], s, level), level)
        if len(ct) == 3:
            out = oc.add(out, oc.multiply(ct[2], oc.multiply(s, s, level), level), level)
        return out

    # -- key-switching keys ------------------------------------------------------------------------------------------------------------
    def _randomness(self, tag, new_key):
        rng = self._rng("ksk", tag)
        a = np.stack([self._uniform(rng, self.primes) for _ in range(self.dnum)])
        e = np.stack([self._residues(rng.integers(-3, 4, self.n), self.primes) for _ in range(self.dnum)])
        return np.ascontiguousarray(new_key[:self.size_q]), a, e

    def relin_randomness(self):
        """(new_key = s^2 [Q][N] in NTT form, a [dnum][QP][N], e [dnum][QP][N] in coefficient form)."""
        s = self.sk_ntt[:self.size_q]
        return self._randomness("relin", self.oc.multiply(s, s, self.size_q))

    def galois_randomness(self, elt):
        return self._randomness(int(elt), self.sk_galois_ntt(elt))

    def oracle_key(self, elt=None):
        """The key of Galois element `elt` (None: the relinearisation key) made by the oracle, [dnum][2][QP][N]."""
        if elt not in self._evk:
            new_key, a, e = self.relin_randomness() if elt is None else self.galois_randomness(elt)
            e_ntt = np.stack([self._ntt(e[d], self.size_qp) for d in range(self.dnum)])
            self._evk[elt] = self.oc.gen_kswitch_key(self.sk_ntt, new_key, a, e_ntt)
        return self._evk[elt]

    def digits(self, elt, level):
        evk = self.oracle_key(elt)
        return [evk[i] for i in range(self.tool(level).beta)]


class CpuCodec:
    """The numpy restatement of the encoder with its own root table."""

    def __init__(self, sch):
        self.sch = sch
        self.roots = R.roots_table(2 * sch.n)
        self.group = R.group_table(2 * sch.n, sch.n // 4)

    def encode(self, z, level, scale, with_special=False):
        """z [count][slots] -> uint64 [count][level (+ size_P)][N], NTT form."""
        sch, out = self.sch, []
        rows = sch.rows(level, with_special)
        for row in np.atleast_2d(z):
            coeffs = R.encode_coeffs(row, sch.slots, self.roots, self.group, scale)
            res = R.residues(R.round_coeffs(coeffs), [sch.primes[r] for r in rows])
            out.append(sch.oc.nwt_forward_map(res, rows))
        return np.stack(out)

    def decode(self, pt, level, scale):
        """uint64 [count][level][N] in NTT form -> complex [count][slots]."""
        sch, out = self.sch, []
        for p in pt:
            coeff = sch.oc.nwt_backward(np.ascontiguousarray(p), level, 0)
            out.append(R.decode_values(R.compose_array(coeff, sch.primes[:level], 1.0 / scale), sch.slots, self.roots, self.group))
        return np.stack(out)


class GpuCodec:
    """The library's CKKSEncoder behind the same two calls; every destination is poisoned first."""

    POISON = -0x2152411021524111

    def __init__(self, sch, P, ctx, enc, device):
        self.sch, self.P, self.ctx, self.enc, self.device = sch, P, ctx, enc, device

    def encode_device(self, z, level, scale, with_special=False):
        import torch
        z = np.array(z, dtype=np.complex128, ndmin=2)            # a writable copy: the inputs may be read-only views
        limbs = level + (self.ctx.size_P if with_special else 0)
        dst = torch.full((z.shape[0], limbs, self.ctx.n), self.POISON, dtype=torch.int64, device=self.device)
        self.enc.encode_batched(level, torch.from_numpy(z).to(self.device), z.shape[1], scale, dst, with_special=with_special)
        return dst

    def encode(self, z, level, scale, with_special=False):
        return self.P.to_host(self.encode_device(z, level, scale, with_special))

    def decode(self, pt, level, scale):
        import torch
        d = self.P.to_device(np.ascontiguousarray(pt), self.device)
        out = torch.full((d.shape[0], self.sch.slots), complex(np.nan, np.nan), dtype=torch.complex128, device=self.device)
        self.enc.decode_batched(level, d, scale, out)
        return out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def scheme(name):
    return Scheme(name)


@functools.lru_cache(maxsize=None)
def cpu_codec(name):
    return CpuCodec(scheme(name))


# ---- the cases: the same inputs, expected values and wrong answers for the oracle pipeline and the GPU pipeline ------------------------
class Result:
    def __init__(self, label, got, want, wrongs=()):
        self.label, self.got, self.want, self.wrongs = label, np.asarray(got), np.asarray(want), list(wrongs)
        self.err = max_err(self.got, self.want)
        self.wrong = nearest_wrong(self.got, self.wrongs) if self.wrongs else None


def _enc(sch, codec, z, level, scale, tag):
    """Encode and encrypt every row of z; tags tag.0, tag.1, ... name the encryption randomness."""
    pts = codec.encode(z, level, scale)
    return [sch.encrypt(pts[k], level, f"{tag}.{k}") for k in range(len(pts))]


def _dec(sch, codec, cts, level, scale):
    return codec.decode(np.stack([sch.decrypt(ct, level) for ct in cts]), level, scale)


def case_rotation(sch, codec, rotate, level, scale, step):
    """rotate(ct, level, elt) -> ct.  step None: conjugation (element 2N - 1)."""
    z = messages(11, 1, sch.slots)
    ct = _enc(sch, codec, z, level, scale, "rot")[0]
    elt = 2 * sch.n - 1 if step is None else elt_of_step(step, sch.n)
    got = _dec(sch, codec, [rotate(ct, level, elt)], level, scale)[0]
    if step is None:
        return Result("conjugate", got, np.conj(z[0]), [z[0], np.roll(z[0], -1), np.roll(z[0], 1)])
    return Result(f"rotate {step}", got, np.roll(z[0], -step), rotation_wrongs(z[0], step))


def case_products(sch, codec, multiply_many, level, scale, batch, square=False):
    """multiply_many(list of a, list of b, level) -> list of [2][level - 1][N] (relinearised and rescaled); square: b is a."""
    z = messages(12, 2 * batch, sch.slots)
    a = _enc(sch, codec, z[:batch], level, scale, "mul.a")
    b = a if square else _enc(sch, codec, z[batch:], level, scale, "mul.b")
    z2 = z[:batch] if square else z[batch:]
    out = multiply_many(a, b, level)
    got = _dec(sch, codec, out, level - 1, scale * scale / float(sch.primes[level - 1]))
    wrongs = [np.stack(w) for w in zip(*[product_wrongs(z[k], z2[k]) for k in range(batch)])]
    if square:
        wrongs = [w for i, w in enumerate(wrongs) if i not in (0, 1)] + [z[:batch]]
    return Result("square" if square else "product", got, z[:batch] * z2, wrongs)


def case_inner_product(sch, codec, inner, level, scale, terms, groups, shared):
    """inner(a [groups][terms] ciphertexts, b [groups][terms] or, shared, [terms], level) -> [groups] ciphertexts at level - 1."""
    za = messages(13, groups * terms, sch.slots).reshape(groups, terms, -1)
    zb = messages(14, groups * terms, sch.slots).reshape(groups, terms, -1)
    a = [_enc(sch, codec, za[g], level, scale, f"ip.a{g}") for g in range(groups)]
    if shared:
        zb = np.broadcast_to(zb[0], zb.shape)
        b = _enc(sch, codec, zb[0], level, scale, "ip.b0")
    else:
        b = [_enc(sch, codec, zb[g], level, scale, f"ip.b{g}") for g in range(groups)]
    got = _dec(sch, codec, inner(a, b, level), level - 1, scale * scale / float(sch.primes[level - 1]))
    want = np.sum(za * zb, axis=1)
    return Result("inner product" + (" (operand 2 shared)" if shared else ""), got, want,
                  [np.sum(za * np.conj(zb), axis=1), (za * zb)[:, 0], np.sum(za[::-1] * zb, axis=1)])


def case_plain_sum(sch, codec, plain_sum, level, scale, terms, groups, with_acc):
    """plain_sum(plain [groups][terms][level][N], ct [groups][terms], acc [groups] or None, level) -> [groups] ciphertexts at level - 1."""
    zp = messages(15, groups * terms, sch.slots).reshape(groups, terms, -1)
    zc = messages(16, groups * terms, sch.slots).reshape(groups, terms, -1)
    zacc = messages(17, groups, sch.slots)
    plain = [codec.encode(zp[g], level, scale) for g in range(groups)]
    ct = [_enc(sch, codec, zc[g], level, scale, f"ps.c{g}") for g in range(groups)]
    acc = _enc(sch, codec, zacc, level, scale * scale, "ps.acc") if with_acc else None
    got = _dec(sch, codec, plain_sum(plain, ct, acc, level), level - 1, scale * scale / float(sch.primes[level - 1]))
    want = np.sum(zp * zc, axis=1) + (zacc if with_acc else 0)
    return Result("plain sum" + (" + acc" if with_acc else ""), got, want, [np.sum(zp * zc, axis=1) + (0 if with_acc else zacc),
                                                                            np.sum(zp * np.conj(zc), axis=1) + (zacc if with_acc else 0)])


def case_hoisting(sch, codec, hoist_many, level, scale, steps, batch):
    """hoist_many(list of ct, level, elts) -> list of ct."""
    z = messages(18, batch, sch.slots)
    ct = _enc(sch, codec, z, level, scale, "hoist")
    got = _dec(sch, codec, hoist_many(ct, level, [elt_of_step(s, sch.n) for s in steps]), level, scale)
    return Result(f"hoisting {list(steps)}", got, sum(np.roll(z, -s, axis=1) for s in steps),
                  [sum(np.roll(z, s, axis=1) for s in steps), len(steps) * z, sum(np.conj(np.roll(z, -s, axis=1)) for s in steps)])


def case_matvec(sch, codec, matvec_many, level, scale, d, batch):
    """matvec_many(list of ct, level, matrix, elts, scale) -> list of ct at level - 1 (weighted hoisting of the d diagonals, rescaled)."""
    m = matrix(d, d, d)
    tv = [periodic(100 * d + b, d, sch.slots) for b in range(batch)]
    ct = _enc(sch, codec, np.stack([t for t, _ in tv]), level, scale, f"mv{d}")
    out = matvec_many(ct, level, m, [elt_of_step(s, sch.n) for s in range(d)], scale)
    got = _dec(sch, codec, out, level - 1, scale * scale / float(sch.primes[level - 1]))
    want = np.stack([np.tile(m @ v, sch.slots // d) for _, v in tv])
    wrongs = [np.stack(w) for w in zip(*[matvec_wrongs(m, v, sch.slots) for _, v in tv])]
    return Result(f"diag matvec {d} x {d}", got, want, wrongs)


def _bsgs_elts(sch, n_baby, n_giant):
    return [elt_of_step(j, sch.n) for j in range(n_baby)], [elt_of_step(i * n_baby, sch.n) for i in range(n_giant)]


def case_bsgs(sch, codec, bsgs_many, level, scale, n_baby, n_giant, batch, prepare=bsgs_diagonals):
    """bsgs_many(list of ct, level, baby elts, giant elts, weights [n_giant][n_baby] slot vectors, scale) -> list of ct at level - 1."""
    d = n_baby * n_giant
    m = matrix(1000 + d, d, d)
    tv = [periodic(200 * d + b, d, sch.slots) for b in range(batch)]
    ct = _enc(sch, codec, np.stack([t for t, _ in tv]), level, scale, f"bsgs{d}")
    baby, giant = _bsgs_elts(sch, n_baby, n_giant)
    out = bsgs_many(ct, level, baby, giant, prepare(m, sch.slots, n_baby, n_giant), scale)
    got = _dec(sch, codec, out, level - 1, scale * scale / float(sch.primes[level - 1]))
    want = np.stack([np.tile(m @ v, sch.slots // d) for _, v in tv])
    wrongs = [np.stack(w) for w in zip(*[matvec_wrongs(m, v, sch.slots) for _, v in tv])]
    wrongs.append(np.stack([bsgs_apply(bsgs_diagonals_without_roll_back(m, sch.slots, n_baby, n_giant), t, n_baby) for t, _ in tv]))
    return Result(f"bsgs matvec {n_baby} x {n_giant}", got, want, wrongs)


def case_bsgs_blocks(sch, codec, bsgs_blocks, level, scale, n_baby, n_giant, n_blocks, prepare=bsgs_diagonals):
    """Row blocks of a (n_blocks d) x d matrix against one vector: bsgs_blocks(ct, level, baby, giant, [weights per block], scale) ->
    one ciphertext at level - 1 per block."""
    d = n_baby * n_giant
    m = matrix(2000 + d, n_blocks * d, d)
    t, v = periodic(300 * d, d, sch.slots)
    ct = _enc(sch, codec, t[None], level, scale, f"blocks{d}")[0]
    baby, giant = _bsgs_elts(sch, n_baby, n_giant)
    blocks = [m[r * d:(r + 1) * d] for r in range(n_blocks)]
    out = bsgs_blocks(ct, level, baby, giant, [prepare(blk, sch.slots, n_baby, n_giant) for blk in blocks], scale)
    got = _dec(sch, codec, out, level - 1, scale * scale / float(sch.primes[level - 1]))
    want = np.stack([np.tile(blk @ v, sch.slots // d) for blk in blocks])
    wrongs = [np.stack(w) for w in zip(*[matvec_wrongs(blk, v, sch.slots) for blk in blocks])]
    wrongs.append(want[::-1])
    return Result(f"bsgs blocks {n_blocks} of {d} x {d}", got, want, wrongs)


def case_config4(sch, codec, relin_rotate_many, level, scale, batch):
    """relin_rotate_many(list of size-3 products [3][level][N], level, elt) -> list of ct at the same level, scale^2."""
    z = messages(19, 2 * batch, sch.slots)
    a = _enc(sch, codec, z[:batch], level, scale, "c4.a")
    b = _enc(sch, codec, z[batch:], level, scale, "c4.b")
    ct3 = [sch.oc.tensor_prod_2x2(x, y, level) for x, y in zip(a, b)]
    got = _dec(sch, codec, relin_rotate_many(ct3, level, elt_of_step(1, sch.n)), level, scale * scale)
    zz = z[:batch] * z[batch:]
    return Result("relinearize + rotate 1", got, np.roll(zz, -1, axis=1), [np.roll(zz, 1, axis=1), zz, np.conj(np.roll(zz, -1, axis=1)),
                                                                         np.roll(z[:batch], -1, axis=1)])


HOST_KEY_STEPS = (1, 2, 4, -1)


def case_host_api(sch, codec, api, scale):
    """The evaluator-level operations (the reference's names; host/phantom.h through pyPhantom on the GPU) at the top level.  `api`:
    rotate(ct, step, with_conjugation_key), hoisting(ct, steps), multiply_relin_rescale(a, b), add, sub, negate, add_plain(ct, pt),
    multiply_plain(ct, pt), mod_switch_to(ct, chain_index) -- ciphertexts as numpy in, (numpy ciphertext, limbs, scale) out.  Galois
    keys exist for HOST_KEY_STEPS only (plus conjugation where asked), so steps 3 = 4 - 1 and 5 = 4 + 1 go through the NAF loop."""
    level = sch.size_q
    z = messages(20, 3, sch.slots)
    a, b = _enc(sch, codec, z[:2], level, scale, "host")
    pt = codec.encode(z[2:], level, scale)[0]
    out = []

    def check(label, res, want, wrongs, limbs=level, want_scale=scale):
        ct, got_limbs, got_scale = res
        assert got_limbs == limbs and ct.shape[1] == limbs, f"{label}: {got_limbs} limbs, want {limbs}"
        assert got_scale == want_scale, f"{label}: scale {got_scale}, want {want_scale}"
        out.append(Result(label, _dec(sch, codec, [ct], limbs, want_scale)[0], want, wrongs))

    for step in (1, -1, 3, 5):
        partial = {3: (-1, 4, 5), 5: (1, 4, 3)}.get(step, ())        # one NAF term alone, or the second one with the wrong sign
        check(f"rotate {step}", api.rotate(a, step, False), np.roll(z[0], -step), rotation_wrongs(z[0], step) +
              [np.roll(z[0], -t) for t in partial])
    check("rotate 0", api.rotate(a, 0, True), np.conj(z[0]), [z[0], np.roll(z[0], -1)])
    check("hoisting [1, 2, 4]", api.hoisting(a, [1, 2, 4]), sum(np.roll(z[0], -s) for s in (1, 2, 4)),
          [sum(np.roll(z[0], s) for s in (1, 2, 4)), 3 * z[0]])
    check("multiply_relin_rescale", api.multiply_relin_rescale(a, b), z[0] * z[1], product_wrongs(z[0], z[1]), level - 1,
          scale * scale / float(sch.primes[level - 1]))
    check("add", api.add(a, b), z[0] + z[1], [z[0] - z[1], z[0]])
    check("sub", api.sub(a, b), z[0] - z[1], [z[1] - z[0], z[0] + z[1]])
    check("negate", api.negate(a), -z[0], [z[0], -np.conj(z[0])])
    check("add_plain", api.add_plain(a, pt), z[0] + z[2], [z[0] - z[2], z[0]])
    check("multiply_plain", api.multiply_plain(a, pt), z[0] * z[2], product_wrongs(z[0], z[2]), level, scale * scale)
    check("mod_switch_to", api.mod_switch_to(a, 3), z[0], [np.conj(z[0]), 0 * z[0]], level - 2, scale)
    return out


def naf(value):
    """Non-adjacent form of a rotation step as signed powers of two, lowest first (the test's own statement)."""
    out, sign, value, i = [], -1 if value < 0 else 1, abs(value), 0
    while value:
        zi = 2 - (value & 3) if value & 1 else 0
        value = (value - zi) >> 1
        if zi:
            out.append(sign * zi * (1 << i))
        i += 1
    return out


class Reference:
    """The operations of the cases composed from oracle steps on numpy ciphertexts (the CPU pipeline); weights are encoded by `codec`."""

    def __init__(self, sch, codec):
        self.sch, self.oc, self.codec = sch, sch.oc, codec

    def add_ct(self, a, b, level):
        return np.stack([self.oc.add(a[p], b[p], level) for p in range(len(a))])

    def rotate(self, ct, level, elt):
        sch = self.sch
        tab = O.galois_ntt_table(sch.log_n, int(elt))
        c0, c1 = (O.apply_galois_ntt(ct[p], tab, sch.n, level) for p in range(2))
        return sch.tool(level).keyswitch_inplace(np.stack([c0, np.zeros_like(c0)]), c1, sch.digits(int(elt), level), O.CKKS)

    def relinearize(self, ct3, level):
        return self.sch.tool(level).keyswitch_inplace(ct3[:2], ct3[2], self.sch.digits(None, level), O.CKKS)

    def rescale(self, ct, level):
        return self.sch.tool(level).rescale_ntt(ct, len(ct))

    def multiply_many(self, a, b, level):
        """tensor product (the squaring form where b is a), relinearise, rescale."""
        return [self.rescale(self.relinearize(self.oc.tensor_square_2x2(x, level) if y is x else self.oc.tensor_prod_2x2(x, y, level), level),
                             level) for x, y in zip(a, b)]

    def inner(self, a, b, level):
        out = []
        for g, row in enumerate(a):
            other, t3 = (b[g] if isinstance(b[0], list) else b), None
            for x, y in zip(row, other):
                t = self.oc.tensor_prod_2x2(x, y, level)
                t3 = t if t3 is None else self.add_ct(t3, t, level)
            out.append(self.rescale(self.relinearize(t3, level), level))
        return out

    def plain_sum(self, plain, ct, acc, level):
        out = []
        for g in range(len(ct)):
            total = None if acc is None else acc[g]
            for p, c in zip(plain[g], ct[g]):
                t = np.stack([self.oc.multiply(c[i], np.ascontiguousarray(p[:level]), level) for i in range(2)])
                total = t if total is None else self.add_ct(total, t, level)
            out.append(self.rescale(total, level))
        return out

    def hoist_many(self, cts, level, elts):
        tool = self.sch.tool(level)
        return [tool.hoisting(ct, elts, [self.sch.digits(e, level) for e in elts], O.CKKS) for ct in cts]

    def _keys(self, elts, level):
        return [None if e == 1 else self.sch.digits(e, level) for e in elts]

    def matvec_many(self, cts, level, m, elts, scale):
        weights = self.codec.encode(matrix_diagonals(m, self.sch.slots), level, scale, with_special=True)
        tool = self.sch.tool(level)
        return [self.rescale(tool.hoisting_weighted(ct, elts, self._keys(elts, level), list(weights), O.CKKS), level) for ct in cts]

    def _bsgs_weights(self, values, level, scale):
        flat = self.codec.encode(np.stack([w for row in values for w in row]), level, scale, with_special=True)
        nb = len(values[0])
        return [[flat[i * nb + j] for j in range(nb)] for i in range(len(values))]

    def bsgs_many(self, cts, level, baby, giant, values, scale):
        weights, tool = self._bsgs_weights(values, level, scale), self.sch.tool(level)
        return [self.rescale(tool.hoisting_weighted_bsgs(ct, baby, self._keys(baby, level), giant, self._keys(giant, level), weights, O.CKKS),
                             level) for ct in cts]

    def bsgs_blocks(self, ct, level, baby, giant, blocks, scale):
        return [self.bsgs_many([ct], level, baby, giant, values, scale)[0] for values in blocks]

    def relin_rotate_many(self, ct3s, level, elt):
        return [self.rotate(self.relinearize(ct3, level), level, elt) for ct3 in ct3s]


class ReferenceHost:
    """case_host_api's `api` from oracle steps: rotations by a step without a key go through the NAF of the step, as the reference's
    rotate_internal does."""

    def __init__(self, ref, scale):
        self.ref, self.sch, self.scale, self.level = ref, ref.sch, scale, ref.sch.size_q

    def _same(self, ct):
        return ct, self.level, self.scale

    def rotate(self, ct, step, with_conjugation_key):
        n = self.sch.n
        if step == 0:
            return self._same(self.ref.rotate(ct, self.level, 2 * n - 1) if with_conjugation_key else ct)
        for t in ([step] if step in HOST_KEY_STEPS else naf(step)):
            assert t in HOST_KEY_STEPS
            ct = self.ref.rotate(ct, self.level, elt_of_step(t, n))
        return self._same(ct)

    def hoisting(self, ct, steps):
        return self._same(self.ref.hoist_many([ct], self.level, [elt_of_step(s, self.sch.n) for s in steps])[0])

    def multiply_relin_rescale(self, a, b):
        return self.ref.multiply_many([a], [b], self.level)[0], self.level - 1, self.scale * self.scale / float(self.sch.primes[self.level - 1])

    def add(self, a, b):
        return self._same(self.ref.add_ct(a, b, self.level))

    def sub(self, a, b):
        return self._same(np.stack([self.sch.oc.sub(a[p], b[p], self.level) for p in range(2)]))

    def negate(self, a):
        return self._same(np.stack([self.sch.oc.negate(a[p], self.level) for p in range(2)]))

    def add_plain(self, a, pt):
        return self._same(np.stack([self.sch.oc.add(a[0], pt, self.level), a[1]]))

    def multiply_plain(self, a, pt):
        return np.stack([self.sch.oc.multiply(a[p], pt, self.level) for p in range(2)]), self.level, self.scale * self.scale

    def mod_switch_to(self, a, chain_index):
        limbs = self.level - (chain_index - 1)
        return np.ascontiguousarray(a[:, :limbs]), limbs, self.scale


# ---- config 4 as BASELINE states it, in BFV: exact ----------------------------------------------------------------------------------------
class BfvConfig4:
    """Two genuine BFV encryptions at c1_bfv4096 (t = 65537), their BEHZ product (and the square of the first), relinearised and
    mapped through X -> X^elt; decrypts to (m1 m2)(X^elt) mod (X^N + 1, t) exactly.  Ciphertexts in coefficient form."""

    NAME, T, ELT, EVERY = "c1_bfv4096", 65537, 5, 53

    def __init__(self):
        self.sch = sch = Scheme(self.NAME, seed=7)
        self.q = [int(p) for p in sch.primes[:sch.size_q]]
        self.big_q = self.q[0] * self.q[1]
        rng = sch._rng("bfv.m")
        self.m = rng.integers(0, self.T, (2, sch.n))
        self.ct = [self.encrypt(self.m[k], k) for k in range(2)]

    def encrypt(self, m, tag):
        sch, oc, L = self.sch, self.sch.oc, self.sch.size_q
        rng = sch._rng("bfv.enc", tag)
        a = sch._uniform(rng, self.q)
        e = rng.integers(-3, 4, sch.n)
        delta = self.big_q // self.T
        dm = np.stack([np.array([(delta * int(v) + int(ev)) % p for v, ev in zip(m, e)], dtype=np.uint64) for p in self.q])
        a_s = oc.nwt_backward(oc.multiply(oc.nwt_forward(a, L, 0), sch.sk_ntt[:L], L), L)
        return np.stack([oc.sub(dm, a_s, L), a])

    def decrypt(self, ct):
        """Every EVERY-th plaintext coefficient of a size-2 ciphertext in coefficient form."""
        from util import crt_compose
        sch, oc, L = self.sch, self.sch.oc, self.sch.size_q
        c1s = oc.nwt_backward(oc.multiply(oc.nwt_forward(ct[1], L, 0), sch.sk_ntt[:L], L), L)
        phase = oc.add(ct[0], c1s, L)
        out = []
        for k in range(0, sch.n, self.EVERY):
            v, _ = crt_compose([phase[l, k] for l in range(L)], self.q)
            out.append(((v * self.T + self.big_q // 2) // self.big_q) % self.T)
        return out

    def want(self, k1, k2):
        """(m_k1 m_k2)(X^ELT) mod (X^N + 1, t) on every EVERY-th coefficient, from the schoolbook product in exact int64."""
        n, t = self.sch.n, self.T
        a, b = self.m[k1].astype(np.int64), self.m[k2].astype(np.int64)
        prod = np.zeros(n, dtype=np.int64)              # |sums| < N t^2 < 2^46: exact in int64
        for i in range(n):                              # negacyclic schoolbook product, one shifted row at a time
            prod[i:] += a[i] * b[:n - i]
            prod[:i] -= a[i] * b[n - i:]
        out = [0] * n
        for i in range(n):
            at = i * self.ELT % (2 * n)
            out[at % n] = int(-prod[i] if at >= n else prod[i]) % t
        return [out[k] for k in range(0, n, self.EVERY)]

    def oracle(self, k1, k2):
        """BEHZ multiply -> relinearise -> Galois (coefficient form) -> key switch, from oracle steps."""
        sch, L = self.sch, self.sch.size_q
        tool = sch.tool(L)
        prod = O.Behz(sch.oc, self.T).multiply(self.ct[k1], self.ct[k2])
        ct = tool.keyswitch_inplace(prod[:2], prod[2], sch.digits(None, L), O.BFV)
        c0, c1 = (sch.oc.apply_galois_coeff(ct[p], self.ELT, L) for p in range(2))
        return tool.keyswitch_inplace(np.stack([c0, np.zeros_like(c0)]), c1, sch.digits(self.ELT, L), O.BFV)
