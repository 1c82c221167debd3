"""Batched BFV multiply at the config-4 shape (N = 2^15, 30 data limbs, t = 1032193): per-op milliseconds of
  (a) a loop of B calls of the single-pair entry, and
  (b) one call of the batched entry,
for BEHZ, HPS and HPS-over-Q at B = 1 .. 64, timed with device events after warm-up, in one process, the two legs alternating, with the
fraction of the 8 TB/s HBM roofline beside each figure (the algorithmic-byte formulas of bench.py's bfv_multiply rows).  The two
legs' outputs are compared word for word before anything is timed.

  --single-only          leg (a) alone: what a build without the batched entries can run (the baseline of the parent commit:
                         point --pkg at that build's phantom-fhe_amd directory)
  --chunk-sweep B        per-op time of the batched entry at batch B for chunk = 1, 2, 4, ... (the default-chunk choice)
  --one VARIANT B        one untimed warm-up and ONE batched call, nothing else (for a kernel trace)
  --json PATH            also write the rows as JSON
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--pkg", default=os.path.join(ROOT, "phantom-fhe_amd"))
ap.add_argument("--variants", default="behz,hps,overq")
ap.add_argument("--batches", default="1,2,4,8,16,32,64")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--single-only", action="store_true")
ap.add_argument("--chunk-sweep", type=int, default=0)
ap.add_argument("--one", nargs=2, metavar=("VARIANT", "B"))
ap.add_argument("--json", default="")
args = ap.parse_args()
sys.path.insert(0, args.pkg)

import torch  # noqa: E402
import phantom_fhe_amd as P  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("time_bfv_batched needs a HIP device: there is nothing to time on a CPU")

PEAK_HBM = 8.0e12
LOG_N, N, SIZE_Q, SIZE_P, PLAIN_T = 15, 1 << 15, 30, 15, 1032193
dev = torch.device("cuda:0")
primes = [int(p) for p in P.coeff_modulus_create(N, [60] + [50] * 29 + [60] * 15)]
ctx = P.PhantomContext(LOG_N, primes, SIZE_P, device=dev)
ctx.set_plain_modulus(PLAIN_T)


def algorithmic_bytes(variant):
    """bench.py's formulas (limb-polynomials of N x 8 B, every stage reads its inputs once and writes its outputs once); over-Q is
    the HPS sequence with |Rl| = |Q|."""
    nq, nbsk = SIZE_Q, SIZE_Q + 2
    nr = SIZE_Q + 1 if variant == "hps" else SIZE_Q
    if variant == "behz":
        units = 4 * (2 * nq + (nq + nbsk + 1) + (2 * nbsk + 1) + 2 * nbsk) + 7 * (nq + nbsk) + 6 * (nq + nbsk) + 3 * (nq + 2 * nbsk) + 3 * (nbsk + nq)
    else:
        units = 4 * ((nq + nr) + 2 * (nq + nr)) + 7 * (nq + nr) + 6 * (nq + nr) + 3 * (nq + 2 * nr) + 3 * (nr + nq)
    return units * 8.0 * N


def single_fn(variant):
    return {"behz": ctx.bfv_multiply_behz, "hps": ctx.bfv_multiply_hps, "overq": ctx.bfv_multiply_hps_overq}[variant]


def batched_call(variant, d1, d2, dst, chunk=0):
    if variant == "behz":
        ctx.bfv_multiply_behz_batched(d1, d2, dst, chunk)
    elif variant == "hps":
        ctx.bfv_multiply_hps_batched(d1, d2, dst, chunk)
    else:
        ctx.bfv_multiply_hps_overq_batched(SIZE_Q, d1, d2, dst, chunk)


def inputs(batch, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    d = torch.empty((batch, 2, SIZE_Q, N), dtype=torch.int64, device=dev)
    for i in range(SIZE_Q):
        d[:, :, i] = torch.randint(0, primes[i], (batch, 2, N), dtype=torch.int64, device=dev, generator=g)
    return d


def timed_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def row(variant, batch, leg, per_op):
    med, best = statistics.median(per_op), min(per_op)
    return {"variant": variant, "B": batch, "leg": leg, "ms_per_op_median": round(med, 5), "ms_per_op_min": round(best, 5),
            "frac_of_8TBs_median": round(algorithmic_bytes(variant) / (med * 1e-3) / PEAK_HBM, 4), "windows": len(per_op)}


def show(r):
    print(f"{r['variant']:6s} B={r['B']:<3d} {r['leg']:22s} {r['ms_per_op_median']:.4f} ms/op (min {r['ms_per_op_min']:.4f})  "
          f"frac {r['frac_of_8TBs_median']:.3f}", flush=True)


rows = []
if args.one:
    variant, batch = args.one[0], int(args.one[1])
    d1, d2 = inputs(batch, 1), inputs(batch, 2)
    dst = torch.zeros((batch, 3, SIZE_Q, N), dtype=torch.int64, device=dev)
    batched_call(variant, d1, d2, dst)       # builds the auxiliary tables and grows the arena
    torch.cuda.synchronize()
    batched_call(variant, d1, d2, dst)
    torch.cuda.synchronize()
    print(f"one batched {variant} call at B={batch} (after one warm-up call)")
    sys.exit(0)

for variant in args.variants.split(","):
    one = single_fn(variant)
    batches = [args.chunk_sweep] if args.chunk_sweep else [int(b) for b in args.batches.split(",")]
    for batch in batches:
        d1, d2 = inputs(batch, 1), inputs(batch, 2)
        dst_a = torch.zeros((batch, 3, SIZE_Q, N), dtype=torch.int64, device=dev)
        dst_b = torch.zeros_like(dst_a)

        def leg_a():
            for b in range(batch):
                one(d1[b], d2[b], dst_a[b])

        legs = [("single-pair loop", leg_a)]
        if args.chunk_sweep:
            legs = []
            c = 1
            while c <= batch:
                legs.append((f"batched chunk={c}", lambda c=c: batched_call(variant, d1, d2, dst_b, c)))
                c *= 2
        elif not args.single_only:
            legs.append(("batched", lambda: batched_call(variant, d1, d2, dst_b)))
        for _, fn in legs:                      # warm-up: tables, arenas, code objects; then the two results must agree
            fn()
            fn()
        torch.cuda.synchronize()
        if not args.single_only:
            if args.chunk_sweep:
                leg_a()
                torch.cuda.synchronize()
            if not torch.equal(dst_a, dst_b):
                sys.exit(f"{variant} B={batch}: the batched result differs from the single-pair loop")
        iters = max(2, -(-96 // batch))         # about 100 multiplies per window
        per_op = {name: [] for name, _ in legs}
        for _ in range(args.reps):              # alternate the legs
            for name, fn in legs:
                per_op[name].append(timed_ms(fn, iters) / batch)
        for name, _ in legs:
            rows.append(row(variant, batch, name, per_op[name]))
            show(rows[-1])
        del d1, d2, dst_a, dst_b
        torch.cuda.empty_cache()

print(json.dumps({"tool": "time_bfv_batched", "device": torch.cuda.get_device_name(0), "rows": rows}))
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
