"""Restatement of PhantomBatchEncoder (src/batchencoder.cu) for the tests: the index map from the reference's loop
(populate_matrix_reps_index_map, :25-49), encode as encode_gpu's scatter (:51-60) followed by the oracle's one-prime inverse transform,
decode as the forward transform followed by decode_gpu's gather (:91-95).  tests/test_batch_restatement.py pins it on the definition
(the plaintext evaluated at psi^(5^i) and psi^-(5^i) gives the slots)."""
import functools

import numpy as np

from oracle import oracle as O

# batching primes of N = 2^12 (t = 1 mod 2^13), one per width the tests walk
LADDER = {16: 40961, 17: 65537, 20: 1032193, 33: 8589852673, 50: 1125899906826241, 51: 2251799813554177, 59: 576460752303415297}


def reverse_bits(x, bits):
    r = 0
    for i in range(bits):
        r |= ((x >> i) & 1) << (bits - 1 - i)
    return r


def index_map(log_n):
    """matrix_reps_index_map: slot i of the first row sits at the bit-reversed (5^i - 1) / 2, slot i of the second row at the
    bit-reversed (2N - 5^i - 1) / 2."""
    return _index_map(log_n).copy()


@functools.lru_cache(maxsize=None)
def _index_map(log_n):
    slots = 1 << log_n
    row, m = slots >> 1, slots << 1
    temp = np.zeros(slots, dtype=np.uint64)
    pos = 1
    for i in range(row):
        temp[i] = reverse_bits((pos - 1) >> 1, log_n)
        temp[row | i] = reverse_bits((m - pos - 1) >> 1, log_n)
        pos = (pos * 5) & (m - 1)
    return temp


def batching_prime(log_n, bits):
    """The prime of `bits` bits the tests use at degree 2^log_n: the ladder at 2^12, the largest such prime = 1 (mod 2N) elsewhere."""
    return LADDER[bits] if log_n == 12 else int(O.get_primes(1 << log_n, bits, 1)[0])


def smallest_batching_prime(log_n):
    """The smallest prime = 1 (mod 2N)."""
    step = 2 << log_n
    t = step + 1
    while not O.is_prime(t):
        t += step
    return t


class Batch:
    def __init__(self, log_n, t):
        self.log_n, self.n, self.t = log_n, 1 << log_n, int(t)
        self.oc = O.Ctx(log_n, [self.t], 0)
        self.map = index_map(log_n).astype(np.int64)

    def sign_rule(self, values):
        v = np.ascontiguousarray(values).view(np.uint64) if np.asarray(values).dtype == np.int64 else np.asarray(values, dtype=np.uint64)
        return v + (v >> np.uint64(63)) * np.uint64(self.t)      # wraps like the kernel's 64-bit words

    def nwt_forward(self, poly):
        return self.oc.nwt_forward(np.asarray(poly, dtype=np.uint64), 1, 0)

    def nwt_backward(self, poly):
        return self.oc.nwt_backward(np.asarray(poly, dtype=np.uint64), 1, 0)

    def encode(self, values):
        """values: up to N words (uint64, or int64 whose negatives take the sign rule) -> the plaintext [N] below t."""
        v = self.sign_rule(values)
        buf = np.zeros(self.n, dtype=np.uint64)
        buf[self.map[:len(v)]] = v
        return self.nwt_backward(buf)

    def decode(self, plain):
        return self.nwt_forward(plain)[self.map]

    def multiply(self, a, b):
        """The negacyclic product of two plaintexts modulo t."""
        prod = self.oc.multiply(self.nwt_forward(a), self.nwt_forward(b), 1, 0).reshape(-1)
        return self.nwt_backward(prod)

    def galois(self, plain, elt):
        return self.oc.apply_galois_coeff(np.asarray(plain, dtype=np.uint64), int(elt), 1, 0).reshape(-1)


@functools.lru_cache(maxsize=None)
def batch(log_n, t):
    return Batch(log_n, t)
