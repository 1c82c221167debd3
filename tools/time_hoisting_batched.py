"""Timing of the batched hoisted rotations (pha_hoisting_batched, pha_hoisting_weighted_batched) at the C3 set (N = 2^16, 45 + 15
limbs, beta = 3) with 16 keyed rotations (+ the identity in the weighted form): per-ciphertext time of the batched entry at
B = 1, 2, 4, 8, 16 next to a loop of B single calls measured in the same session (development helper; profiles/hoisting_batched.md).

    python tools/time_hoisting_batched.py                 the table: median of 5 samples per side, taken alternately, each >= ~300 ms of calls
    python tools/time_hoisting_batched.py --trace plain   3 batched calls at B = 8 and nothing else, for a kernel trace of its own
                                                          (rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/... --trace plain)
"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "phantom-fhe_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import phantom_fhe_amd as P
from util import primes_of

log_n, primes, size_p = primes_of("c3_ckks16")
n = 1 << log_n
size_q = len(primes) - size_p
dev = torch.device("cuda:0")
ctx = P.PhantomContext(log_n, list(primes), size_p, device=dev)
gen = torch.Generator(device=dev); gen.manual_seed(1)
def rnd(*shape):
    return torch.randint(0, 1 << 49, shape, generator=gen, device=dev, dtype=torch.int64)   # below every prime
dnum = size_q // size_p
CK = P.scheme_type.ckks
N_ROT = 16
rot = [pow(5, j + 1, 2 * n) for j in range(N_ROT)]
keys = [P.PhantomRelinKey([rnd(2, len(primes), n) for _ in range(dnum)]) for _ in rot]
weights = [rnd(size_q + size_p, n) for _ in range(N_ROT + 1)]
FORMS = {
    "plain": (lambda ct, out, chunk: ctx.hoisting_batched(size_q, ct, rot, keys, CK, out=out, chunk=chunk),
              lambda ct: ctx.hoisting(size_q, ct, rot, keys, CK)),
    "weighted": (lambda ct, out, chunk: ctx.hoisting_weighted_batched(size_q, ct, [1] + rot, [None] + keys, weights, CK, out=out, chunk=chunk),
                 lambda ct: ctx.hoisting_weighted(size_q, ct, [1] + rot, [None] + keys, weights, CK)),
}


def sample(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def measure_pair(fa, fb, samples=5, target_ms=300.0):
    """Median, min and max of `samples` timings of each of two callables, taken alternately in one session."""
    reps = []
    for fn in (fa, fb):
        for _ in range(2):
            fn()                               # warm-up: tables, scratch arena, clocks
        reps.append(max(2, int(target_ms / max(sample(fn, 1), 1e-3))))
    ta, tb = [], []
    for _ in range(samples):
        ta.append(sample(fa, reps[0]))
        tb.append(sample(fb, reps[1]))
    ta.sort(); tb.sort()
    return (ta[len(ta) // 2], ta[0], ta[-1]), (tb[len(tb) // 2], tb[0], tb[-1])


if len(sys.argv) > 2 and sys.argv[1] == "--trace":
    batched, _ = FORMS[sys.argv[2]]
    ct = rnd(8, 2, size_q, n)
    out = torch.empty_like(ct)
    for _ in range(3):
        batched(ct, out, 0)
    torch.cuda.synchronize()
    sys.exit(0)

print(f"C3 set: N = 2^{log_n}, {size_q} + {size_p} limbs, beta = {ctx.beta(size_q)}, {N_ROT} keyed rotations; ms per ciphertext, "
      "median (min .. max) of 5 samples", flush=True)
for form, (batched, single) in FORMS.items():
    for B in (1, 2, 4, 8, 16):
        ct = rnd(B, 2, size_q, n)
        out = torch.empty_like(ct)
        work = ct.clone()
        def loop():
            for b in range(B):
                single(work[b])
        (lm, llo, lhi), (bm, blo, bhi) = measure_pair(loop, lambda: batched(ct, out, 0))
        print(f"{form:8s} B = {B:2d}: loop of single calls {lm / B:7.3f} ({llo / B:.3f} .. {lhi / B:.3f})   batched {bm / B:7.3f} "
              f"({blo / B:.3f} .. {bhi / B:.3f})   batched / loop = {bm / lm:.3f}", flush=True)
        del ct, out, work
