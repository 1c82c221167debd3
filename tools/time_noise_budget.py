"""The invariant noise budget of a batch of bfv ciphertexts on raw buffers: milliseconds per call of
  budget   pha_invariant_noise_budget_batched (PHA_SCHEME_BFV): phase, exact norm of t * phase, budget, all on the device,
  decrypt  pha_bfv_decrypt_batched on the same batch (the same phase, then the scale-and-round instead of the norm),
  norm     pha_poly_infty_norm_batched alone on a buffer of `batch` phases with scalar = t (the two launches the budget adds),
  round    pha_hps_decrypt_scale_and_round on ONE phase (times batch in the table: the step the norm takes the place of),
and seconds per ciphertext of
  host     what a user did before: the phase from the earlier entries (forward transforms, pha_decrypt_phase_batched, inverse
           transform), a copy to the host, the CRT in Python object arrays and the norm there (one ciphertext, one repetition; its
           budget must equal the device's).
Shape: N = 2^15, 30 + 15 limbs (c4), size_Ql = 15 and 30, batch 8, t = 65537, uniform ciphertexts (the work does not depend on the
words).  Device events after warm-up, one process, the legs alternating; median, minimum and spread over the windows.  Derived
next to the measured: modular multiply-subtracts per coefficient of the norm, L (L - 1) / 2.

  --levels 15,30             size_Ql, comma separated
  --batch B                  ciphertexts per call (default 8)
  --reps R                   windows per leg (default 7)
  --no-host                  skip the host leg
  --json PATH                also write the rows as JSON
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--pkg", default=os.path.join(ROOT, "phantom-fhe_amd"))
ap.add_argument("--levels", default="15,30")
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--no-host", action="store_true")
ap.add_argument("--json", default="")
args = ap.parse_args()
sys.path.insert(0, args.pkg)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import phantom_fhe_amd as P  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("time_noise_budget needs a HIP device: there is nothing to time on a CPU")

PLAIN_T = 65537
BFV = int(P.scheme_type.bfv)
LOG_N, BITS, SIZE_P = 15, [60] + [50] * 29 + [60] * 15, 15
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


def host_budget(ctx, primes, ql, n, ct, sk):
    """One ciphertext [2][ql][N] in coefficient form -> (budget, seconds), the way of tests/bv_semantics.py."""
    t0 = time.perf_counter()
    work = ct.clone()
    for p in range(2):
        ctx.nwt_2d_radix8_forward_inplace(work[p], ql, 0)
    phase = torch.empty((1, ql, n), dtype=torch.int64, device=dev)
    ctx.decrypt_phase_batched(ql, work[None], sk, phase)
    ctx.nwt_2d_radix8_backward_inplace(phase[0], ql, 0)
    coeff = P.to_host(phase[0])
    q = [int(p) for p in primes[:ql]]
    big = math.prod(q)
    acc = np.zeros(n, dtype=object)
    for i, p in enumerate(q):
        mi = big // p
        acc = acc + coeff[i].astype(object) * (mi * pow(mi, -1, p) % big)
    v = acc % big * PLAIN_T % big
    worst = max(min(int(x), big - int(x)) for x in v)
    budget = max(0, big.bit_length() - worst.bit_length() - 1)
    return budget, time.perf_counter() - t0


def run_level(ctx, primes, ql, n, batch, reps, with_host):
    gen = torch.Generator(device=dev)
    gen.manual_seed(100 + ql)
    ct = uniform((batch, 2), primes[:ql], n, gen)
    phases = uniform((batch,), primes[:ql], n, gen)
    sk = ctx.secret_key_powers(uniform((), primes, n, gen), 1)
    budget = torch.empty((batch,), dtype=torch.int32, device=dev)
    bits = torch.empty((batch,), dtype=torch.int32, device=dev)
    plain = torch.empty((batch, n), dtype=torch.int64, device=dev)
    one = torch.empty((n,), dtype=torch.int64, device=dev)
    legs = [("budget", lambda: ctx.invariant_noise_budget_batched(ql, ct, sk, BFV, budget)),
            ("decrypt", lambda: ctx.bfv_decrypt_batched(ql, ct, sk, plain)),
            ("norm", lambda: ctx.poly_infty_norm_batched(ql, phases, bits, scalar=PLAIN_T)),
            ("round", lambda: ctx.hps_decrypt_scale_and_round(ql, one, phases[0]))]
    for _, fn in legs:                       # warm-up: code objects, tables, arenas
        fn()
        fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in legs}
    iters = {name: max(3, int(60.0 / max(timed_ms(fn, 2), 1e-3))) for name, fn in legs}   # windows of about 60 ms
    for _ in range(reps):                    # alternate the legs
        for name, fn in legs:
            ms[name].append(timed_ms(fn, iters[name]))
    rows = []
    for name, _ in legs:
        med, lo, hi = statistics.median(ms[name]), min(ms[name]), max(ms[name])
        per = 1 if name == "round" else batch
        rows.append({"ql": ql, "B": batch, "leg": name, "ms_median": round(med, 5), "ms_min": round(lo, 5),
                     "us_per_item": round(1000.0 * med / per, 3), "spread_pct": round(100.0 * (hi - lo) / med, 2), "windows": len(ms[name]),
                     "iters_per_window": iters[name]})
        r = rows[-1]
        print(f"ql={ql:<2d} B={batch:<2d} {name:8s} {r['ms_median']:9.4f} ms per call = {r['us_per_item']:.2f} us per "
              f"{'polynomial' if name == 'round' else 'ciphertext'} (min {r['ms_min']:.4f} ms, spread {r['spread_pct']:.1f} %)", flush=True)
    by = {r["leg"]: r for r in rows}
    derived = {"ql": ql, "B": batch, "leg": "derived", "garner_mulsubs_per_coeff": ql * (ql - 1) // 2,
               "budget_over_decrypt": round(by["budget"]["ms_median"] / by["decrypt"]["ms_median"], 3),
               "norm_over_round": round(by["norm"]["ms_median"] / (by["round"]["ms_median"] * batch), 3)}
    print(f"ql={ql:<2d} B={batch:<2d} budget / decrypt {derived['budget_over_decrypt']:.3f}; norm / (batch x round) {derived['norm_over_round']:.3f}; "
          f"{derived['garner_mulsubs_per_coeff']} multiply-subtracts per coefficient (derived)", flush=True)
    rows.append(derived)
    if with_host:
        want, seconds = host_budget(ctx, primes, ql, n, ct[0], sk)
        got = int(budget[0].item())
        if got != want:
            sys.exit(f"ql={ql}: the device's budget {got} differs from the host's {want}")
        rows.append({"ql": ql, "B": 1, "leg": "host", "s_per_ct": round(seconds, 3), "budget": want,
                     "host_over_budget_per_ct": round(seconds * 1e6 / by["budget"]["us_per_item"], 1)})
        print(f"ql={ql:<2d} host leg {seconds:.3f} s per ciphertext (one repetition; budget {want} on both sides) = "
              f"{rows[-1]['host_over_budget_per_ct']:.0f} x the entry's time per ciphertext", flush=True)
    return rows


n = 1 << LOG_N
primes = [int(p) for p in P.coeff_modulus_create(n, BITS)]
ctx = P.PhantomContext(LOG_N, primes, SIZE_P, device=dev).set_plain_modulus(PLAIN_T)
rows = []
for ql in [int(v) for v in args.levels.split(",")]:
    rows += run_level(ctx, primes, ql, n, args.batch, args.reps, not args.no_host)
    torch.cuda.empty_cache()
out = {"tool": "time_noise_budget", "device": torch.cuda.get_device_name(0), "rows": rows}
print(json.dumps(out))
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
