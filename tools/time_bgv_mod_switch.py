"""BGV relinearize + mod_switch_to_next on raw buffers: milliseconds per call of
  fused    pha_keyswitch_mod_switch_batched (ONE call, ct only read),
  two-call what the library offered before and the host mirror still does for mod_switch_to_next(relinearize(...)): a device copy
           of ct, pha_keyswitch_inplace_batched(..., BGV) on the copy, pha_mod_t_and_divide_q_last_ntt on it (same bits, checked
           before timing).
Shapes: N = 2^15 with 30 + 15 limbs at ql = 30 (c4) and N = 2^16 with 45 + 15 limbs at ql = 45 (c3), batch 1, 8 and 16, plain
modulus 786433.  Device events after warm-up, one process, the legs alternating; median, minimum and spread over the windows.

  --shapes c4:1,c3:8         config:batch, comma separated (default: the six above)
  --reps R                   windows per leg (default 7)
  --one LEG:SHAPE            one warm-up and ONE call of that leg (fused or two-call), nothing else: run it under
                             `rocprofv3 --kernel-trace --stats` for the kernels of that path with their times
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
ap.add_argument("--shapes", default="c4:1,c4:8,c4:16,c3:1,c3:8,c3:16")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--one", default="")
ap.add_argument("--json", default="")
args = ap.parse_args()
sys.path.insert(0, args.pkg)

import torch  # noqa: E402
import phantom_fhe_amd as P  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("time_bgv_mod_switch needs a HIP device: there is nothing to time on a CPU")

PLAIN_T = 786433
BGV = int(P.scheme_type.bgv)
SETS = {   # name -> (log N, bit sizes of QP, special primes)
    "c4": (15, [60] + [50] * 29 + [60] * 15, 15),
    "c3": (16, [60] + [50] * 44 + [60] * 15, 15),
}
dev = torch.device("cuda:0")


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


def run_shape(ctx, rlk, primes, ql, n, set_name, batch, reps, one):
    gen = torch.Generator(device=dev)
    gen.manual_seed(100 + batch)
    ct = uniform((batch, 2), primes[:ql], n, gen)
    c2 = uniform((batch,), primes[:ql], n, gen)
    work = torch.empty_like(ct)
    dst_f = torch.empty((batch, 2, ql - 1, n), dtype=torch.int64, device=dev)
    dst_t = torch.empty_like(dst_f)
    keys = rlk.public_keys_ptr

    def fused():
        ctx.keyswitch_mod_switch_batched(ql, ct, c2, batch, keys, dst_f)

    def two_call():
        work.copy_(ct)
        ctx.keyswitch_inplace_batched(ql, work, c2, batch, keys, BGV)
        ctx.mod_t_and_divide_q_last_ntt(ql, work, 2 * batch, dst_t)

    legs = [("fused", fused), ("two-call", two_call)]
    if one:
        fn = dict(legs)[one]
        fn()
        torch.cuda.synchronize()
        fn()
        torch.cuda.synchronize()
        print(f"one {one} call at {set_name} B={batch} (after one warm-up call)")
        return []
    for _, fn in legs:                       # warm-up: code objects, tables, arenas
        fn()
        fn()
    torch.cuda.synchronize()
    if not torch.equal(dst_f, dst_t):
        sys.exit(f"{set_name} B={batch}: the fused entry differs from the two calls")
    ms = {name: [] for name, _ in legs}
    iters = {name: max(3, int(60.0 / max(timed_ms(fn, 2), 1e-3))) for name, fn in legs}   # windows of about 60 ms
    for _ in range(reps):                    # alternate the legs
        for name, fn in legs:
            ms[name].append(timed_ms(fn, iters[name]))
    rows = []
    for name, _ in legs:
        med, lo, hi = statistics.median(ms[name]), min(ms[name]), max(ms[name])
        rows.append({"set": set_name, "B": batch, "leg": name, "ms_median": round(med, 5), "ms_min": round(lo, 5),
                     "ms_per_ct": round(med / batch, 5), "spread_pct": round(100.0 * (hi - lo) / med, 2), "windows": len(ms[name]),
                     "iters_per_window": iters[name]})
        r = rows[-1]
        print(f"{set_name} B={batch:<2d} {name:9s} {r['ms_median']:9.4f} ms = {r['ms_per_ct']:.4f} per ciphertext (min {r['ms_min']:.4f}, "
              f"spread {r['spread_pct']:.1f} %)", flush=True)
    ratio = {"set": set_name, "B": batch, "leg": "ratio", "two_call_over_fused": round(rows[1]["ms_median"] / rows[0]["ms_median"], 4)}
    print(f"{set_name} B={batch:<2d} two-call / fused {ratio['two_call_over_fused']:.3f}", flush=True)
    return rows + [ratio]


rows = []
one_leg = ""
shapes = args.shapes.split(",")
if args.one:
    one_leg, shape = args.one.split(":", 1)
    if one_leg not in ("fused", "two-call"):
        sys.exit("--one takes fused:SHAPE or two-call:SHAPE")
    shapes = [shape]
contexts = {}
for shape in shapes:
    set_name, batch = shape.split(":")
    batch = int(batch)
    if set_name not in contexts:
        contexts.clear()                     # one set's tables and keys at a time
        torch.cuda.empty_cache()
        log_n, bits, size_p = SETS[set_name]
        n = 1 << log_n
        primes = [int(p) for p in P.coeff_modulus_create(n, bits)]
        ctx = P.PhantomContext(log_n, primes, size_p, device=dev).set_plain_modulus(PLAIN_T)
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
    rows += run_shape(ctx, rlk, primes, ql, n, set_name, batch, args.reps, one_leg)
    torch.cuda.empty_cache()

if not args.one:
    out = {"tool": "time_bgv_mod_switch", "device": torch.cuda.get_device_name(0), "rows": rows}
    print(json.dumps(out))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
