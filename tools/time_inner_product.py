"""Encrypted inner products sum_k a_k * b_k (CKKS, multiply + relinearize + rescale): milliseconds per call of
  kernel   pha_tensor_prod_2x2_sum_batched alone (the summed tensor product, one launch),
  entry    pha_inner_product_relin_rescale_batched (that kernel + ONE batched key switch per sum),
against the two compositions the library offered before, built only from entries this tool does not otherwise use:
  lazy-sum K x pha_tensor_prod_2x2_batched and (K - 1) rounds of three pha_add_rns_poly per group (the summed kernel's counterpart),
  lazy     lazy-sum followed by one pha_keyswitch_rescale_batched (the entry's counterpart; same bits, checked before timing),
  eager    K x (pha_tensor_prod_2x2_batched + pha_keyswitch_rescale_batched) and the (K - 1) rounds of adds of the results.
Shapes: the config-3 set (N = 2^16, 45 data limbs + 15 special) at K = 2, 8, 32 with one group and K = 8 with 8 groups sharing
operand 2, and c2_ckks14 (N = 2^14, 8 + 1 limbs) at K = 8.  Device events after warm-up, one process, the legs alternating;
median, minimum and spread over the windows.  For the kernel also the achieved bytes/s over its algorithmic bytes,
(4 K + 3) L N 8 per group (a shared operand counted once per group), and the fraction of the 8 TB/s HBM peak.

  --shapes c3:2:1,c3:8:8     config:terms:groups, comma separated (default: the five above)
  --reps R                   windows per leg (default 7)
  --one SHAPE                one warm-up and ONE call of the entry, nothing else (for a kernel trace)
  --json PATH                also write the rows as JSON
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--pkg", default=os.path.join(ROOT, "phantom-fhe_amd"))
ap.add_argument("--shapes", default="c3:2:1,c3:8:1,c3:32:1,c3:8:8,c2:8:1")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--one", default="")
ap.add_argument("--json", default="")
args = ap.parse_args()
sys.path.insert(0, args.pkg)

import torch  # noqa: E402
import phantom_fhe_amd as P  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("time_inner_product needs a HIP device: there is nothing to time on a CPU")

PEAK_HBM = 8.0e12
SETS = {   # name -> (log N, bit sizes of QP, special primes)
    "c3": (16, [60] + [50] * 44 + [60] * 15, 15),
    "c2": (14, [60] + [40] * 7 + [60], 1),
}
dev = torch.device("cuda:0")


def kernel_bytes(terms, groups, ql, n):
    return groups * (4 * terms + 3) * ql * n * 8.0


def uniform(shape_front, primes, n, gen):
    """[*shape_front][2][L][N] uniform residues."""
    d = torch.empty((*shape_front, 2, len(primes), n), dtype=torch.int64, device=dev)
    for i, q in enumerate(primes):
        d[..., i, :] = torch.randint(0, q, (*shape_front, 2, n), dtype=torch.int64, device=dev, generator=gen)
    return d


def timed_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def run_shape(ctx, rlk, primes, ql, n, set_name, terms, groups, reps, one):
    gen = torch.Generator(device=dev)
    gen.manual_seed(1000 * terms + groups)
    data = primes[:ql]
    op1 = uniform((groups, terms), data, n, gen)                      # [G][K][2][L][N]
    vec = uniform((terms,), data, n, gen)                             # [K][2][L][N], shared when groups > 1
    shared = groups > 1
    op2 = vec if shared else vec[None]
    s01 = torch.empty((groups, 2, ql, n), dtype=torch.int64, device=dev)
    s2 = torch.empty((groups, ql, n), dtype=torch.int64, device=dev)
    dst = torch.empty((groups, 2, ql - 1, n), dtype=torch.int64, device=dev)
    keys = rlk.public_keys_ptr

    def kernel():
        ctx.tensor_prod_2x2_sum_batched(op1, op2, s01, s2, ql, terms, groups)

    def entry():
        ctx.inner_product_relin_rescale_batched(ql, op1, op2, terms, groups, keys, dst)

    if one:
        entry()
        torch.cuda.synchronize()
        entry()
        torch.cuda.synchronize()
        print(f"one inner_product_relin_rescale_batched call at {set_name} K={terms} G={groups} (after one warm-up call)")
        return []
    # the compositions get the layout their entries want: term-major operands, operand 2 replicated per group
    a_t = op1.transpose(0, 1).contiguous()                            # [K][G][2][L][N]
    b_t = vec[:, None].expand(terms, groups, 2, ql, n).contiguous()
    acc01, acc2 = torch.empty_like(s01), torch.empty_like(s2)
    tmp01, tmp2 = torch.empty_like(s01), torch.empty_like(s2)
    dst_a = torch.empty_like(dst)
    dst_b, tmp_b = torch.empty_like(dst), torch.empty_like(dst)

    def lazy_sum():
        ctx.tensor_prod_2x2_batched(a_t[0], b_t[0], acc01, acc2, ql, groups)
        for k in range(1, terms):
            ctx.tensor_prod_2x2_batched(a_t[k], b_t[k], tmp01, tmp2, ql, groups)
            for g in range(groups):
                ctx.add_rns_poly(acc01[g, 0], tmp01[g, 0], acc01[g, 0], ql, 0)
                ctx.add_rns_poly(acc01[g, 1], tmp01[g, 1], acc01[g, 1], ql, 0)
                ctx.add_rns_poly(acc2[g], tmp2[g], acc2[g], ql, 0)

    def lazy():
        lazy_sum()
        ctx.keyswitch_rescale_batched(ql, acc01, acc2, groups, keys, dst_a)

    def eager():
        for k in range(terms):
            ctx.tensor_prod_2x2_batched(a_t[k], b_t[k], tmp01, tmp2, ql, groups)
            ctx.keyswitch_rescale_batched(ql, tmp01, tmp2, groups, keys, dst_b if k == 0 else tmp_b)
            if k:
                for g in range(groups):
                    ctx.add_rns_poly(dst_b[g, 0], tmp_b[g, 0], dst_b[g, 0], ql - 1, 0)
                    ctx.add_rns_poly(dst_b[g, 1], tmp_b[g, 1], dst_b[g, 1], ql - 1, 0)

    legs = [("kernel", kernel), ("lazy-sum", lazy_sum), ("entry", entry), ("lazy", lazy), ("eager", eager)]
    for _, fn in legs:                       # warm-up: code objects, tables, arenas
        fn()
        fn()
    torch.cuda.synchronize()
    if not (torch.equal(s01, acc01) and torch.equal(s2, acc2)):
        sys.exit(f"{set_name} K={terms} G={groups}: the summed kernel differs from tensor products + adds")
    if not torch.equal(dst, dst_a):
        sys.exit(f"{set_name} K={terms} G={groups}: the entry differs from the lazy composition")
    ms = {name: [] for name, _ in legs}
    iters = {name: max(3, int(60.0 / max(timed_ms(fn, 2), 1e-3))) for name, fn in legs}   # windows of about 60 ms
    for _ in range(reps):                    # alternate the legs
        for name, fn in legs:
            ms[name].append(timed_ms(fn, iters[name]))
    rows = []
    for name, _ in legs:
        med, lo, hi = statistics.median(ms[name]), min(ms[name]), max(ms[name])
        r = {"set": set_name, "K": terms, "G": groups, "leg": name, "ms_median": round(med, 5), "ms_min": round(lo, 5),
             "spread_pct": round(100.0 * (hi - lo) / med, 2), "windows": len(ms[name]), "iters_per_window": iters[name]}
        if name == "kernel":
            rate = kernel_bytes(terms, groups, ql, n) / (med * 1e-3)
            r["algorithmic_MB"] = round(kernel_bytes(terms, groups, ql, n) / 1e6, 1)
            r["TB_per_s"] = round(rate / 1e12, 3)
            r["frac_of_8TBs"] = round(rate / PEAK_HBM, 4)
        rows.append(r)
    med = {r["leg"]: r["ms_median"] for r in rows}
    ratios = {"set": set_name, "K": terms, "G": groups, "leg": "ratios",
              "lazy_sum_over_kernel": round(med["lazy-sum"] / med["kernel"], 3),
              "lazy_over_entry": round(med["lazy"] / med["entry"], 3),
              "eager_over_entry": round(med["eager"] / med["entry"], 3)}
    for r in rows:
        extra = f"  {r['TB_per_s']:.3f} TB/s = {r['frac_of_8TBs']:.3f} of 8 TB/s" if "TB_per_s" in r else ""
        print(f"{set_name} K={terms:<3d} G={groups:<2d} {r['leg']:9s} {r['ms_median']:9.4f} ms (min {r['ms_min']:.4f}, spread "
              f"{r['spread_pct']:.1f} %){extra}", flush=True)
    print(f"{set_name} K={terms:<3d} G={groups:<2d} ratios    lazy-sum / kernel {ratios['lazy_sum_over_kernel']:.2f}   lazy / entry "
          f"{ratios['lazy_over_entry']:.2f}   eager / entry {ratios['eager_over_entry']:.2f}", flush=True)
    return rows + [ratios]


rows = []
shapes = [args.one] if args.one else args.shapes.split(",")
contexts = {}
for shape in shapes:
    set_name, terms, groups = shape.split(":")
    terms, groups = int(terms), int(groups)
    if set_name not in contexts:
        contexts.clear()                     # one set's tables and keys at a time
        torch.cuda.empty_cache()
        log_n, bits, size_p = SETS[set_name]
        n = 1 << log_n
        primes = [int(p) for p in P.coeff_modulus_create(n, bits)]
        ctx = P.PhantomContext(log_n, primes, size_p, device=dev)
        ql = len(primes) - size_p
        gen = torch.Generator(device=dev)
        gen.manual_seed(7)
        dnum = -(-ql // size_p)
        evk = torch.empty((dnum, 2, len(primes), n), dtype=torch.int64, device=dev)   # synthetic uniform keys
        for i, q in enumerate(primes):
            evk[:, :, i] = torch.randint(0, q, (dnum, 2, n), dtype=torch.int64, device=dev, generator=gen)
        rlk = P.PhantomRelinKey([evk[i] for i in range(dnum)])
        del evk
        contexts[set_name] = (ctx, rlk, primes, ql, n)
    ctx, rlk, primes, ql, n = contexts[set_name]
    rows += run_shape(ctx, rlk, primes, ql, n, set_name, terms, groups, args.reps, bool(args.one))
    torch.cuda.empty_cache()

if not args.one:
    out = {"tool": "time_inner_product", "device": torch.cuda.get_device_name(0), "rows": rows}
    print(json.dumps(out))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
