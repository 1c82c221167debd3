"""Timing of the batched baby-step / giant-step hoisted rotations (pha_hoisting_weighted_bsgs_batched) at the C3 set (N = 2^16,
45 + 15 limbs, level 45, beta = 3, CKKS) for the splits 16 x 8 and 64 x 2 of a 128-diagonal block: per-ciphertext time of the
batched entry at B = 1, 2, 4, 8 next to a loop of B single pha_hoisting_weighted_bsgs calls measured in the same session
(development helper; profiles/bsgs_batched.md).  Keys cycle over 3 buffers and weights over 4, as tests/test_gpu_workloads.py does
(the launches, pointer tables and accumulations are the real ones).

    python tools/time_bsgs_batched.py [16x8 64x2]       the table: median of 5 samples per side, taken alternately, each >= ~300 ms of calls
    python tools/time_bsgs_batched.py --trace 16x8      3 batched calls at B = 4 and nothing else, for a kernel trace of its own
                                                        (rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/... --trace 16x8)
    python tools/time_bsgs_batched.py --trace 16x8 single   the same for 3 x 4 single calls
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
key_pool = [P.PhantomRelinKey([rnd(2, len(primes), n) for _ in range(dnum)]) for _ in range(3)]
w_pool = [rnd(size_q + size_p, n) for _ in range(4)]


def operands(nb, ng):
    baby = [pow(5, j, 2 * n) for j in range(nb)]
    giant = [pow(5, nb * i, 2 * n) for i in range(ng)]
    bk = [None] + [key_pool[j % 3] for j in range(1, nb)]
    gk = [None] + [key_pool[(i + 1) % 3] for i in range(1, ng)]
    ws = [[w_pool[(i * nb + j) % 4] for j in range(nb)] for i in range(ng)]
    return baby, bk, giant, gk, ws


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


def parse(a):
    return tuple(int(x) for x in a.split("x"))


if len(sys.argv) > 1 and sys.argv[1] == "--trace":
    nb, ng = parse(sys.argv[2] if len(sys.argv) > 2 else "16x8")
    baby, bk, giant, gk, ws = operands(nb, ng)
    ct = rnd(4, 2, size_q, n)
    out = torch.empty_like(ct)
    for _ in range(3):
        if sys.argv[3:] == ["single"]:         # the loop the table compares with: 4 single calls, in place on a copy
            out.copy_(ct)
            for b in range(4):
                ctx.hoisting_weighted_bsgs(size_q, out[b], baby, bk, giant, gk, ws, CK)
        else:
            ctx.hoisting_weighted_bsgs_batched(size_q, ct, baby, bk, giant, gk, ws, CK, out=out)
    torch.cuda.synchronize()
    sys.exit(0)

print(f"C3 set: N = 2^{log_n}, {size_q} + {size_p} limbs, beta = {ctx.beta(size_q)}; ms per ciphertext, median (min .. max) of 5 samples",
      flush=True)
for nb, ng in [parse(a) for a in (sys.argv[1:] or ["16x8", "64x2"])]:
    baby, bk, giant, gk, ws = operands(nb, ng)
    for B in (1, 2, 4, 8):
        ct = rnd(B, 2, size_q, n)
        out = torch.empty_like(ct)
        work = ct.clone()
        def loop():
            for b in range(B):
                ctx.hoisting_weighted_bsgs(size_q, work[b], baby, bk, giant, gk, ws, CK)
        def batched():
            ctx.hoisting_weighted_bsgs_batched(size_q, ct, baby, bk, giant, gk, ws, CK, out=out)
        (lm, llo, lhi), (bm, blo, bhi) = measure_pair(loop, batched)
        print(f"{nb:2d} x {ng} B = {B}: loop of single calls {lm / B:7.3f} ({llo / B:.3f} .. {lhi / B:.3f})   batched {bm / B:7.3f} "
              f"({blo / B:.3f} .. {bhi / B:.3f})   batched / loop = {bm / lm:.3f}", flush=True)
        del ct, out, work
