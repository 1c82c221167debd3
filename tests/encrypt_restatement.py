"""The reference's encryption sequences (src/secretkey.cu:11-192, 232-295, 382-395, 463-531) restated as compositions of oracle calls, in
the reference's order -- the expected words of tests/test_gpu_encrypt.py, pinned by tests/test_encrypt_restatement.py.

Only oracle steps: nwt_forward / nwt_backward, multiply, multiply_scalar, multiply_and_add, negate, add, bgv_lift_plain, bfv_add_plain,
Tool.moddown.  A polynomial over the rows [0, l) u P is handled as two row ranges, the data rows at table row 0 and the special rows at
table row |Q| (start_idx).  Randomness is an argument everywhere: a sample (the noise e, the ternary u) is [N] small signed integers
shared by every limb and is expanded to residues here, as sample_error_poly / sample_ternary_poly write them; the uniform a is
canonical words taken as NTT form.  k = t for bgv, 1 otherwise."""
import numpy as np

from oracle import oracle as O


def residues(v, primes):
    """[N] signed integers -> [len(primes)][N] canonical residues."""
    v = np.asarray(v, dtype=np.int64)
    return np.stack([np.mod(v, np.int64(int(q))).astype(np.uint64) for q in primes])


class Restatement:
    def __init__(self, oc, scheme, t=0):
        self.oc, self.scheme, self.t = oc, int(scheme), int(t)
        self.primes = [int(q) for q in oc.primes]
        self._tools = {}
        if self.scheme != O.CKKS and not self.t:
            raise ValueError("bgv / bfv need a plain modulus")

    def tool(self, l):
        if l not in self._tools:
            self._tools[l] = O.Tool(self.oc, l)
            if self.t:
                self._tools[l].set_plain_modulus(self.t)
        return self._tools[l]

    # -- the two row ranges of a [rows][N] polynomial -------------------------------------------------------------------------------------
    def ranges(self, l, special):
        """(first buffer row, rows, first table row) of each range."""
        out = [(0, l, 0)]
        if special:
            out.append((l, self.oc.size_p, self.oc.size_q))
        return out

    def row_primes(self, l, special):
        return self.primes[:l] + (self.primes[self.oc.size_q:] if special else [])

    def by_rows(self, x, l, special):
        """The rows [0, l) u P of an array over all QP rows (the key, the public key's polynomials)."""
        x = np.asarray(x)
        return np.concatenate([x[:l], x[self.oc.size_q:]]) if special else np.ascontiguousarray(x[:l])

    def over(self, l, special, fn, *polys):
        """fn(limbs, start_idx, *the rows of each polynomial) per range, the results stacked back to [rows][N]."""
        return np.concatenate([fn(cnt, start, *[np.ascontiguousarray(p[r0:r0 + cnt]) for p in polys]) for r0, cnt, start in self.ranges(l, special)])

    def forward(self, x, l, special):
        return self.over(l, special, lambda cnt, start, p: self.oc.nwt_forward(p, cnt, start), x)

    def backward(self, x, l, special):
        return self.over(l, special, lambda cnt, start, p: self.oc.nwt_backward(p, cnt, start), x)

    def noise(self, v, l, special, scaled):
        """sample_error_poly, then multiply_scalar_rns_poly by t under bgv (scaled), in coefficient form."""
        primes = self.row_primes(l, special)
        e = residues(v, primes)
        if not (scaled and self.scheme == O.BGV):
            return e
        scalar = np.array([self.t % q for q in primes], dtype=np.uint64)
        return self.over(l, special, lambda cnt, start, p, s: self.oc.multiply_scalar(p, s[:, 0], cnt, start), e, scalar[:, None])

    # -- PhantomSecretKey -----------------------------------------------------------------------------------------------------------------
    def zero_symmetric(self, sk_ntt, a, e, l, special=False, ntt_form=True):
        """encrypt_zero_symmetric: a [rows][N], e [N] -> [2][rows][N]."""
        oc = self.oc
        s = self.by_rows(sk_ntt, l, special)
        c1 = np.ascontiguousarray(a)
        if ntt_form:
            u = self.forward(self.noise(e, l, special, True), l, special)
            c0 = self.over(l, special, lambda cnt, start, x, y, d: oc.negate(oc.multiply_and_add(x, y, d, cnt, start), cnt, start), c1, s, u)
            return np.stack([c0, c1])
        u = self.noise(e, l, special, False)
        c0 = self.over(l, special, lambda cnt, start, x, y: oc.multiply(x, y, cnt, start), c1, s)
        c0 = self.backward(c0, l, special)
        c0 = self.over(l, special, lambda cnt, start, x, y: oc.negate(oc.add(x, y, cnt, start), cnt, start), c0, u)
        return np.stack([c0, self.backward(c1, l, special)])

    def public_key(self, sk_ntt, a, e):
        """gen_publickey: the zero encryption at the key level, NTT form, [2][QP][N]."""
        return self.zero_symmetric(sk_ntt, a, e, self.oc.size_q, special=bool(self.oc.size_p), ntt_form=True)

    def add_plain(self, c0, plain, l):
        """The plaintext step of encrypt_symmetric / encrypt_asymmetric on c0 [l][N]."""
        oc = self.oc
        if self.scheme == O.CKKS:
            return oc.add(c0, np.ascontiguousarray(plain), l)
        if self.scheme == O.BGV:
            return oc.add(c0, oc.bgv_lift_plain(plain, l), l)
        return oc.bfv_add_plain(c0, plain, self.t)

    def symmetric(self, sk_ntt, a, e, plain, l):
        ct = self.zero_symmetric(sk_ntt, a, e, l, special=False, ntt_form=self.scheme != O.BFV)
        return np.stack([self.add_plain(ct[0], plain, l), ct[1]])

    # -- PhantomPublicKey -----------------------------------------------------------------------------------------------------------------
    def zero_asymmetric_wide(self, pk, u, e, l):
        """encrypt_zero_asymmetric_internal_internal over the rows [0, l) u P: u [N], e [2][N] -> [2][l + |P|][N]."""
        oc = self.oc
        un = self.forward(residues(u, self.row_primes(l, True)), l, True)
        out = []
        for j in range(2):
            pkj = self.by_rows(pk[j], l, True)
            if self.scheme != O.BFV:
                ci = self.forward(self.noise(e[j], l, True, True), l, True)
                out.append(self.over(l, True, lambda cnt, start, x, y, d: oc.multiply_and_add(x, y, d, cnt, start), un, pkj, ci))
            else:
                ci = self.backward(self.over(l, True, lambda cnt, start, x, y: oc.multiply(x, y, cnt, start), pkj, un), l, True)
                out.append(self.over(l, True, lambda cnt, start, x, y: oc.add(x, y, cnt, start), ci, self.noise(e[j], l, True, False)))
        return np.stack(out)

    def zero_asymmetric(self, pk, u, e, l):
        wide = self.zero_asymmetric_wide(pk, u, e, l)
        return np.stack([self.tool(l).moddown(wide[j], self.scheme) for j in range(2)])

    def asymmetric(self, pk, u, e, plain, l):
        ct = self.zero_asymmetric(pk, u, e, l)
        return np.stack([self.add_plain(ct[0], plain, l), ct[1]])
