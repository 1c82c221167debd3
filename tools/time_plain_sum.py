"""Plaintext-weighted sums of ciphertexts sum_k pt_k (.) ct_k (CKKS, one rescale per sum): milliseconds per call of
  kernel    pha_multiply_plain_sum_batched alone (one launch, the sums in registers),
  entry     pha_plain_inner_product_rescale_batched (that kernel + ONE level drop per sum),
against the same results composed from the entries the library offered before:
  compose-sum  per group and polynomial pha_multiply_rns_poly for the first term and pha_multiply_and_add_rns_poly for every
               further one (2 K launches per group, the running sum read and rewritten K times),
  compose      compose-sum followed by pha_divide_and_round_q_last_ntt over the 2 G polynomials (same bits, checked before timing).
Shapes: the config-3 set (N = 2^16, 45 data limbs + 15 special) at K = 2, 8, 32 with 1 and 8 groups, at K = 8 with 8 groups
sharing ct (rows of a matrix against one vector) or plain (one layer applied to a batch of inputs), and c2_ckks14 (N = 2^14,
8 + 1 limbs) at K = 8.  Device events after warm-up, one process, the legs alternating; median, minimum and spread over the
windows, and whether the slowest window of the new leg still beats the fastest window of its composition.  For the kernel also the
achieved bytes/s over its algorithmic bytes, (3 K + 2) L N 8 per group (a shared operand counted once per group, as the kernel
reads it), and the fraction of the 8 TB/s HBM peak.

  --shapes c3:2:1:d,c3:8:8:c    config:terms:groups:sharing (d distinct, c shared ct, p shared plain), comma separated
  --reps R                      windows per leg (default 7)
  --one SHAPE                   one warm-up and ONE call of the entry, nothing else (for a kernel trace)
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
ap.add_argument("--shapes", default="c3:2:1:d,c3:8:1:d,c3:32:1:d,c3:2:8:d,c3:8:8:d,c3:32:8:d,c3:8:8:c,c3:8:8:p,c2:8:1:d,c2:8:8:d")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--one", default="")
ap.add_argument("--json", default="")
args = ap.parse_args()
sys.path.insert(0, args.pkg)

import torch  # noqa: E402
import phantom_fhe_amd as P  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("time_plain_sum needs a HIP device: there is nothing to time on a CPU")

PEAK_HBM = 8.0e12
CKKS = int(P.scheme_type.ckks)
SETS = {   # name -> (log N, bit sizes of QP, special primes)
    "c3": (16, [60] + [50] * 44 + [60] * 15, 15),
    "c2": (14, [60] + [40] * 7 + [60], 1),
}
dev = torch.device("cuda:0")


def kernel_bytes(terms, groups, ql, n):
    return groups * (3 * terms + 2) * ql * n * 8.0


def uniform(shape_front, primes, n, gen):
    """[*shape_front][L][N] uniform residues."""
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


def run_shape(ctx, primes, ql, n, set_name, terms, groups, sharing, reps, one):
    gen = torch.Generator(device=dev)
    gen.manual_seed(1000 * terms + groups)
    data = primes[:ql]
    plain = uniform((terms,) if sharing == "p" else (groups, terms), data, n, gen)        # [G][K][L][N] or shared [K][L][N]
    ct = uniform((terms, 2) if sharing == "c" else (groups, terms, 2), data, n, gen)      # [G][K][2][L][N] or shared [K][2][L][N]
    res = torch.empty((groups, 2, ql, n), dtype=torch.int64, device=dev)
    dst = torch.empty((groups, 2, ql - 1, n), dtype=torch.int64, device=dev)

    def kernel():
        ctx.multiply_plain_sum_batched(plain, ct, None, res, ql, terms, groups)

    def entry():
        ctx.plain_inner_product_rescale_batched(ql, plain, ct, None, terms, groups, CKKS, dst)

    tag = f"{set_name} K={terms:<3d} G={groups:<2d} {sharing}"
    if one:
        entry()
        torch.cuda.synchronize()
        entry()
        torch.cuda.synchronize()
        print(f"one plain_inner_product_rescale_batched call at {tag} (after one warm-up call)")
        return []
    acc, dst_c = torch.empty_like(res), torch.empty_like(dst)
    pl = (lambda g, k: plain[k]) if sharing == "p" else (lambda g, k: plain[g, k])
    cp = (lambda g, k, p: ct[k, p]) if sharing == "c" else (lambda g, k, p: ct[g, k, p])

    def compose_sum():
        for g in range(groups):
            for p in range(2):
                ctx.multiply_rns_poly(pl(g, 0), cp(g, 0, p), acc[g, p], ql, 0)
                for k in range(1, terms):
                    ctx.multiply_and_add_rns_poly(pl(g, k), cp(g, k, p), acc[g, p], acc[g, p], ql, 0)

    def compose():
        compose_sum()
        ctx.divide_and_round_q_last_ntt(ql, acc, 2 * groups, dst_c)

    legs = [("kernel", kernel), ("compose-sum", compose_sum), ("entry", entry), ("compose", compose)]
    for _, fn in legs:                       # warm-up: code objects, tables, arenas
        fn()
        fn()
    torch.cuda.synchronize()
    if not torch.equal(dst, dst_c):
        sys.exit(f"{tag}: the entry differs from the composition")
    kernel()
    compose_sum()
    torch.cuda.synchronize()
    if not torch.equal(res, acc):
        sys.exit(f"{tag}: the sum kernel differs from multiply + multiply_and_add")
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
        if name == "kernel":
            rate = kernel_bytes(terms, groups, ql, n) / (med * 1e-3)
            r["algorithmic_MB"] = round(kernel_bytes(terms, groups, ql, n) / 1e6, 1)
            r["TB_per_s"] = round(rate / 1e12, 3)
            r["frac_of_8TBs"] = round(rate / PEAK_HBM, 4)
        rows.append(r)
    by = {r["leg"]: r for r in rows}
    ratios = {"set": set_name, "K": terms, "G": groups, "sharing": sharing, "leg": "ratios",
              "compose_sum_over_kernel": round(by["compose-sum"]["ms_median"] / by["kernel"]["ms_median"], 3),
              "compose_over_entry": round(by["compose"]["ms_median"] / by["entry"]["ms_median"], 3),
              # the slowest window of the new leg against the fastest window of the composition: faster beyond the spread
              "kernel_faster_beyond_spread": by["kernel"]["ms_max"] < by["compose-sum"]["ms_min"],
              "entry_faster_beyond_spread": by["entry"]["ms_max"] < by["compose"]["ms_min"]}
    for r in rows:
        extra = f"  {r['algorithmic_MB']:.0f} MB, {r['TB_per_s']:.3f} TB/s = {r['frac_of_8TBs']:.3f} of 8 TB/s" if "TB_per_s" in r else ""
        print(f"{tag} {r['leg']:11s} {r['ms_median']:9.4f} ms = {r['ms_per_sum']:.4f} per sum (min {r['ms_min']:.4f}, max {r['ms_max']:.4f}, "
              f"spread {r['spread_pct']:.1f} %){extra}", flush=True)
    print(f"{tag} ratios      compose-sum / kernel {ratios['compose_sum_over_kernel']:.2f} (beyond spread: "
          f"{ratios['kernel_faster_beyond_spread']})   compose / entry {ratios['compose_over_entry']:.2f} (beyond spread: "
          f"{ratios['entry_faster_beyond_spread']})", flush=True)
    return rows + [ratios]


rows = []
shapes = [args.one] if args.one else args.shapes.split(",")
contexts = {}
for shape in shapes:
    set_name, terms, groups, sharing = shape.split(":")
    terms, groups = int(terms), int(groups)
    if sharing not in ("d", "c", "p") or (sharing != "d" and groups < 2):
        sys.exit(f"{shape}: sharing is d, c or p, and a shared operand needs at least two groups")
    if set_name not in contexts:
        contexts.clear()                     # one set's tables at a time
        torch.cuda.empty_cache()
        log_n, bits, size_p = SETS[set_name]
        n = 1 << log_n
        primes = [int(p) for p in P.coeff_modulus_create(n, bits)]
        ctx = P.PhantomContext(log_n, primes, size_p, device=dev)
        contexts[set_name] = (ctx, primes, len(primes) - size_p, n)
    ctx, primes, ql, n = contexts[set_name]
    rows += run_shape(ctx, primes, ql, n, set_name, terms, groups, sharing, args.reps, bool(args.one))
    torch.cuda.empty_cache()

if not args.one:
    out = {"tool": "time_plain_sum", "device": torch.cuda.get_device_name(0), "rows": rows}
    print(json.dumps(out))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
