"""Batched decryption: microseconds per ciphertext of
  entry     pha_decrypt_phase_batched (ckks) / pha_bfv_decrypt_batched (bfv) / pha_bgv_decrypt_batched (bgv),
against the same result composed from the entries the library offered before, per ciphertext:
  compose   ckks: a device copy of c0 + one pha_multiply_and_add_rns_poly per further polynomial;
            bfv: per further polynomial a copy + pha_nwt_2d_radix8_forward_inplace + pha_multiply_and_add_rns_poly into a zeroed sum,
            pha_nwt_2d_radix8_backward_inplace, pha_add_rns_poly with c0 (the phase; the scale-and-round has no earlier entry and is
            left out of the composition, so the bfv comparison favours the composition by one kernel);
            bgv: the ckks composition, pha_nwt_2d_radix8_backward_inplace, pha_exact_convert_array to t (correction factors 1).
The phases are checked equal before timing (bfv: the entry's words against pha_hps_decrypt_scale_and_round of the composed phase).
Shapes: ckks at c3_ckks16 level 45, bfv and bgv at c4_bfv15 level 30; batch 1 and 8; cipher_size 2 and 3.  Device events after warm-up, one
process, the legs alternating; the median over --reps windows (default 21) of --iters calls each.  Next to the times the derived
words moved per output word of the phase: k + (k - 1) / G + 1 (G = min(batch, 4)) against the composition's 4 (k - 1) + 2.

  --json PATH   also write the rows as JSON
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--pkg", default=os.path.join(ROOT, "phantom-fhe_amd"))
ap.add_argument("--reps", type=int, default=21)
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--json", default="")
args = ap.parse_args()
sys.path.insert(0, args.pkg)

import torch  # noqa: E402
import phantom_fhe_amd as P  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("measure_decrypt needs a HIP device: there is nothing to time on a CPU")

SETS = {   # name -> (log N, bit sizes of QP, special primes, level, plain modulus)
    "ckks": ("c3_ckks16", 16, [60] + [50] * 44 + [60] * 15, 15, 45, 0),
    "bfv": ("c4_bfv15", 15, [60] + [50] * 29 + [60] * 15, 15, 30, 65537),
    "bgv": ("c4_bfv15", 15, [60] + [50] * 29 + [60] * 15, 15, 30, 65537),
}
dev = torch.device("cuda:0")


def uniform(shape_front, primes, n, gen):
    d = torch.empty((*shape_front, len(primes), n), dtype=torch.int64, device=dev)
    for i, q in enumerate(primes):
        d[..., i, :] = torch.randint(0, q, (*shape_front, n), dtype=torch.int64, device=dev, generator=gen)
    return d


def timed_us(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1000.0 * e0.elapsed_time(e1) / iters


rows = []
for scheme, (name, log_n, bits, size_p, level, plain_t) in SETS.items():
    n = 1 << log_n
    primes = [int(p) for p in P.coeff_modulus_create(n, bits)]
    ctx = P.PhantomContext(log_n, primes, size_p, device=dev)
    if plain_t:
        ctx.set_plain_modulus(plain_t)
    gen = torch.Generator(device=dev)
    gen.manual_seed(0xDEC0 + level)
    sk = ctx.secret_key_powers(uniform((), primes, n, gen), 2)
    to_t = P.DBaseConverter(ctx, list(range(level)), out_modulus=plain_t) if scheme == "bgv" else None
    for k in (2, 3):
        for batch in (1, 8):
            ct = uniform((batch, k), primes[:level], n, gen)
            out_words = level * n if scheme == "ckks" else n
            dst = torch.empty((batch, out_words), dtype=torch.int64, device=dev)
            phase = torch.empty((batch, level, n), dtype=torch.int64, device=dev)
            tmp = torch.empty((level, n), dtype=torch.int64, device=dev)

            if scheme == "ckks":
                def entry():
                    ctx.decrypt_phase_batched(level, ct, sk, dst)

                def compose():
                    for b in range(batch):
                        phase[b].copy_(ct[b, 0])
                        for i in range(1, k):
                            ctx.multiply_and_add_rns_poly(ct[b, i], sk[i - 1, :level], phase[b], phase[b], level)
            elif scheme == "bgv":
                want = torch.empty((batch, n), dtype=torch.int64, device=dev)

                def entry():
                    ctx.bgv_decrypt_batched(level, ct, sk, dst)

                def compose():
                    for b in range(batch):
                        phase[b].copy_(ct[b, 0])
                        for i in range(1, k):
                            ctx.multiply_and_add_rns_poly(ct[b, i], sk[i - 1, :level], phase[b], phase[b], level)
                        ctx.nwt_2d_radix8_backward_inplace(phase[b], level, 0)
                        to_t.exact_convert_array(want[b], phase[b])
            else:
                def entry():
                    ctx.bfv_decrypt_batched(level, ct, sk, dst)

                def compose():
                    for b in range(batch):
                        phase[b].zero_()
                        for i in range(1, k):
                            tmp.copy_(ct[b, i])
                            ctx.nwt_2d_radix8_forward_inplace(tmp, level, 0)
                            ctx.multiply_and_add_rns_poly(tmp, sk[i - 1, :level], phase[b], phase[b], level)
                        ctx.nwt_2d_radix8_backward_inplace(phase[b], level, 0)
                        ctx.add_rns_poly(ct[b, 0], phase[b], phase[b], level)

            entry()
            compose()
            torch.cuda.synchronize()
            if scheme == "ckks":
                same = torch.equal(dst.view(batch, level, n), phase)
            elif scheme == "bgv":
                same = torch.equal(dst, want)
            else:
                one = torch.empty((n,), dtype=torch.int64, device=dev)
                same = True
                for b in range(batch):
                    ctx.hps_decrypt_scale_and_round(level, one, phase[b])
                    same = same and torch.equal(one, dst[b])
            for _ in range(3):
                entry()
                compose()
            te, tc = [], []
            for _ in range(args.reps):
                te.append(timed_us(entry, args.iters))
                tc.append(timed_us(compose, args.iters))
            G = min(batch, 4)
            rows.append({"scheme": scheme, "set": name, "level": level, "cipher_size": k, "batch": batch, "same_words": bool(same),
                         "entry_us_per_ct": statistics.median(te) / batch, "compose_us_per_ct": statistics.median(tc) / batch,
                         "entry_min_us": min(te) / batch, "compose_min_us": min(tc) / batch, "entry_max_us": max(te) / batch,
                         "phase_words_entry": k + (k - 1) / G + 1, "phase_words_compose": 4 * (k - 1) + 2})
            r = rows[-1]
            print(f"{scheme:5s} {name:10s} L={level} k={k} B={batch}: entry {r['entry_us_per_ct']:9.2f} us/ct  compose {r['compose_us_per_ct']:9.2f} us/ct  "
                  f"ratio {r['compose_us_per_ct'] / r['entry_us_per_ct']:.2f}  words {r['phase_words_entry']:.2f} vs {r['phase_words_compose']}  "
                  f"same {same}  entry windows {r['entry_min_us']:.2f} .. {r['entry_max_us']:.2f}", flush=True)
    del ctx
    torch.cuda.empty_cache()
print("device:", torch.cuda.get_device_name(0))
if args.json:
    with open(args.json, "w") as f:
        json.dump(rows, f, indent=1)
