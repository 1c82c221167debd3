"""BFV plaintext-weighted sums sum_k pt_k * ct_k (coefficient-form ciphertexts, t = 65537): milliseconds per call of
  sum     pha_bfv_multiply_plain_sum_batched (plaintexts lifted and transformed beforehand: the fixed weights of a model),
  raw     pha_bfv_plain_inner_product_batched (raw plaintexts, lifted and transformed inside the call),
against the only form the library offered before,
  loop    per group and term pha_bfv_multiply_plain (cipher_size 2) and, from the second term on, pha_add_rns_poly per polynomial.
The loop's entries are unchanged by the sums, so its time is also the time of the library without them.  The results are compared
bit for bit before anything is timed (the loop on copies); the timed loop multiplies in place in one scratch copy of ct, without the
copy a caller who keeps ct would pay.
Shapes: the config-4 set (N = 2^15, 30 data limbs + 15 special) at K = 2, 8, 32 for 8 groups with their own ciphertexts and for 8
groups sharing ct (rows of a matrix against one vector).  Device events on the launch stream after warm-up, one process, the legs
alternating; median, minimum and spread over the windows, and whether the slowest window of a new leg still beats the fastest window
of the loop.  Also the achieved bytes/s of `sum` over its algorithmic bytes, (16 K + 16 + 12 K + 8) L N per group -- the
transforms' 16 K + 16 and the sum kernel's 12 K + 8 bytes per coefficient and limb -- and the fraction of the 8 TB/s HBM peak.

  --shapes c4:2:8:d,c4:8:8:c    config:terms:groups:sharing (d distinct, c shared ct), comma separated
  --reps R                      windows per leg (default 7)
  --json PATH                   also write the rows as JSON
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--pkg", default=os.path.join(ROOT, "phantom-fhe_amd"))
ap.add_argument("--shapes", default="c4:2:8:d,c4:8:8:d,c4:32:8:d,c4:2:8:c,c4:8:8:c,c4:32:8:c")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--json", default="")
args = ap.parse_args()
sys.path.insert(0, args.pkg)

import torch  # noqa: E402
import phantom_fhe_amd as P  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("time_bfv_plain_sum needs a HIP device: there is nothing to time on a CPU")

PEAK_HBM = 8.0e12
T = 65537
SETS = {   # name -> (log N, bit sizes of QP, special primes)
    "c4": (15, [60] + [50] * 29 + [60] * 15, 15),
}
dev = torch.device("cuda:0")


def algorithmic_bytes(terms, groups, ql, n, with_acc=False):
    return groups * (16 * terms + 16 + 12 * terms + 8 + (16 if with_acc else 0)) * ql * n * 1.0


def uniform(shape_front, primes, n, gen):
    d = torch.empty((*shape_front, len(primes), n), dtype=torch.int64, device=dev)
    for i, q in enumerate(primes):
        d[..., i, :] = torch.randint(0, q, (*shape_front, n), dtype=torch.int64, device=dev, generator=gen)
    return d


def timed_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def run_shape(ctx, primes, ql, n, set_name, terms, groups, sharing, reps):
    gen = torch.Generator(device=dev)
    gen.manual_seed(2000 * terms + groups)
    data = primes[:ql]
    raw = torch.randint(0, T, (groups, terms, n), dtype=torch.int64, device=dev, generator=gen)
    ct = uniform((terms, 2) if sharing == "c" else (groups, terms, 2), data, n, gen)
    lifted = torch.empty((groups, terms, ql, n), dtype=torch.int64, device=dev)
    ctx.bfv_lift_plain_batched(ql, raw, groups * terms, lifted)
    res, res_raw = (torch.empty((groups, 2, ql, n), dtype=torch.int64, device=dev) for _ in range(2))
    work, acc = ct.clone(), torch.empty((groups, 2, ql, n), dtype=torch.int64, device=dev)
    prod = torch.empty((2, ql, n), dtype=torch.int64, device=dev)
    ct_of = (lambda buf, g, k: buf[k]) if sharing == "c" else (lambda buf, g, k: buf[g, k])

    def leg_sum():
        ctx.bfv_multiply_plain_sum_batched(ql, lifted, ct, None, res, terms, groups)

    def leg_raw():
        ctx.bfv_plain_inner_product_batched(ql, raw, ct, None, res_raw, terms, groups)

    def loop_checked():                      # on copies: the reference result
        for g in range(groups):
            for k in range(terms):
                dst = acc[g] if k == 0 else prod
                dst.copy_(ct_of(ct, g, k))
                ctx.bfv_multiply_plain(ql, dst, 2, raw[g, k])
                if k:
                    for p in range(2):
                        ctx.add_rns_poly(acc[g, p], prod[p], acc[g, p], ql)

    def leg_loop():                          # the same launches without the copies: in place in the scratch copy of ct
        for g in range(groups):
            for k in range(terms):
                c = ct_of(work, g, k)
                ctx.bfv_multiply_plain(ql, c, 2, raw[g, k])
                if k:
                    for p in range(2):
                        ctx.add_rns_poly(acc[g, p], c[p], acc[g, p], ql)

    tag = f"{set_name} K={terms:<3d} G={groups:<2d} {sharing}"
    legs = [("sum", leg_sum), ("raw", leg_raw), ("loop", leg_loop)]
    for _, fn in legs:                       # warm-up: code objects, tables, arenas
        fn()
        fn()
    loop_checked()
    leg_sum()
    leg_raw()
    torch.cuda.synchronize()
    if not (torch.equal(res, acc) and torch.equal(res_raw, acc)):
        sys.exit(f"{tag}: the sum entries differ from the loop")
    ms = {name: [] for name, _ in legs}
    iters = {name: max(3, int(60.0 / max(timed_ms(fn, 2), 1e-3))) for name, fn in legs}   # windows of about 60 ms
    for _ in range(reps):                    # alternate the legs
        for name, fn in legs:
            ms[name].append(timed_ms(fn, iters[name]))
    rows = []
    for name, _ in legs:
        med, lo, hi = statistics.median(ms[name]), min(ms[name]), max(ms[name])
        r = {"set": set_name, "K": terms, "G": groups, "sharing": sharing, "leg": name, "ms_median": round(med, 5), "ms_min": round(lo, 5),
             "ms_max": round(hi, 5), "ms_per_sum": round(med / groups, 5), "spread_pct": round(100.0 * (hi - lo) / med, 2),
             "windows": len(ms[name]), "iters_per_window": iters[name]}
        if name == "sum":
            rate = algorithmic_bytes(terms, groups, ql, n) / (med * 1e-3)
            r["algorithmic_MB"] = round(algorithmic_bytes(terms, groups, ql, n) / 1e6, 1)
            r["TB_per_s"] = round(rate / 1e12, 3)
            r["frac_of_8TBs"] = round(rate / PEAK_HBM, 4)
        rows.append(r)
    by = {r["leg"]: r for r in rows}
    ratios = {"set": set_name, "K": terms, "G": groups, "sharing": sharing, "leg": "ratios",
              "loop_over_sum": round(by["loop"]["ms_median"] / by["sum"]["ms_median"], 3),
              "loop_over_raw": round(by["loop"]["ms_median"] / by["raw"]["ms_median"], 3),
              "sum_faster_beyond_spread": by["sum"]["ms_max"] < by["loop"]["ms_min"],
              "raw_faster_beyond_spread": by["raw"]["ms_max"] < by["loop"]["ms_min"]}
    for r in rows:
        extra = f"  {r['algorithmic_MB']:.0f} MB, {r['TB_per_s']:.3f} TB/s = {r['frac_of_8TBs']:.3f} of 8 TB/s" if "TB_per_s" in r else ""
        print(f"{tag} {r['leg']:5s} {r['ms_median']:9.4f} ms = {r['ms_per_sum']:.4f} per sum (min {r['ms_min']:.4f}, max {r['ms_max']:.4f}, "
              f"spread {r['spread_pct']:.1f} %){extra}", flush=True)
    print(f"{tag} ratios loop / sum {ratios['loop_over_sum']:.2f} (beyond spread: {ratios['sum_faster_beyond_spread']})   "
          f"loop / raw {ratios['loop_over_raw']:.2f} (beyond spread: {ratios['raw_faster_beyond_spread']})", flush=True)
    return rows + [ratios]


rows = []
contexts = {}
for shape in args.shapes.split(","):
    set_name, terms, groups, sharing = shape.split(":")
    terms, groups = int(terms), int(groups)
    if sharing not in ("d", "c") or (sharing != "d" and groups < 2):
        sys.exit(f"{shape}: sharing is d or c, and a shared operand needs at least two groups")
    if set_name not in contexts:
        contexts.clear()                     # one set's tables at a time
        torch.cuda.empty_cache()
        log_n, bits, size_p = SETS[set_name]
        n = 1 << log_n
        primes = [int(p) for p in P.coeff_modulus_create(n, bits)]
        ctx = P.PhantomContext(log_n, primes, size_p, device=dev)
        ctx.set_plain_modulus(T)
        contexts[set_name] = (ctx, primes, len(primes) - size_p, n)
    ctx, primes, ql, n = contexts[set_name]
    rows += run_shape(ctx, primes, ql, n, set_name, terms, groups, sharing, args.reps)
    torch.cuda.empty_cache()

out = {"tool": "time_bfv_plain_sum", "device": torch.cuda.get_device_name(0), "rows": rows}
print(json.dumps(out))
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
