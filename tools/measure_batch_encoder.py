"""BFV / BGV batch encoder: microseconds per message of
  encode            pha_batch_encode_batched with the permutation as the gather of the first pass's load,
  encode-kernel     pha_batch_encode_batched with the permutation kernel followed by the inverse transform,
  decode-scatter    pha_batch_decode_batched with the permutation as the scatter of the last store,
  decode-gather     pha_batch_decode_batched with a plain last store followed by the gather kernel,
against the unfused composition, which is the reference's structure (src/batchencoder.cu): the index permutation as a launch of its
own (torch indexing) plus the plain transform entry, pha_plain_nwt_{backward,forward}_inplace_batched -- the same transform kernels
with no permutation:
  encode-unfused    zero-fill + buf[:, index_map] = values + backward transform in place,
  decode-unfused    copy of the plaintexts + forward transform in place + out = ntt[:, index_map].
Shapes: N = 2^12, 2^15, 2^17; count = 1, 8, 64 (and 32 at 2^17, between the two sides of the encode rule); t = a 17-to-20-bit
batching prime (65537 up to 2^15, 786433 at 2^17) and a 59-bit one.  The words of every form are compared once, on fresh buffers, before anything is timed.  Device events on the launch stream after
warm-up, one process, the forms alternating; the median, minimum and maximum over --reps windows (default 15) of --iters calls each.
Next to the times the algorithmic bytes per message, 16 N (the message read once, the plaintext written once; the tables are shared
by the batch), and the fraction of the 8 TB/s peak that rate is -- a count over a measured time, not a counter reading.

  --json PATH   also write the rows as JSON
  --md PATH     also write the tables as markdown
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--pkg", default=os.path.join(ROOT, "phantom-fhe_amd"))
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--json", default="")
ap.add_argument("--md", default="")
args = ap.parse_args()
sys.path.insert(0, args.pkg)

import torch  # noqa: E402
import phantom_fhe_amd as P  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("measure_batch_encoder needs a HIP device: there is nothing to time on a CPU")

dev = torch.device("cuda:0")
PEAK = 8.0e12
FORMS = ("encode", "encode-kernel", "encode-unfused", "decode-scatter", "decode-gather", "decode-unfused")


def is_prime(v):
    if v < 2 or v % 2 == 0:
        return v == 2
    d, s = v - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        if a % v == 0:
            continue
        x = pow(a, d, v)
        if x in (1, v - 1):
            continue
        for _ in range(s - 1):
            x = x * x % v
            if x == v - 1:
                break
        else:
            return False
    return True


def batching_prime_below(n, bits):
    t = (1 << bits) - 2 * n + 1
    while not is_prime(t):
        t -= 2 * n
    return t


def timed_us(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1000.0 * e0.elapsed_time(e1) / iters


rows = []
for log_n in (12, 15, 17):
    n = 1 << log_n
    primes = [int(p) for p in P.coeff_modulus_create(n, [60, 60])]
    for t in (65537 if log_n <= 15 else 786433, batching_prime_below(n, 59)):
        ctx = P.PhantomContext(log_n, primes, 1, device=dev)
        ctx.set_plain_modulus(t)
        enc = P.BatchEncoder(ctx)
        imap = torch.from_numpy(enc.index_map().astype("int64")).to(dev)
        gen = torch.Generator(device=dev)
        gen.manual_seed(0xBA7C + log_n)
        for count in ((1, 8, 32, 64) if log_n == 17 else (1, 8, 64)):
            values = torch.randint(0, t, (count, n), dtype=torch.int64, device=dev, generator=gen)
            plain, plain_k, plain_u = (torch.empty_like(values) for _ in range(3))
            out_s, out_g, out_u, work = (torch.empty_like(values) for _ in range(4))

            def encode_unfused():
                plain_u.zero_()
                plain_u[:, imap] = values
                enc.plain_nwt_backward_inplace_batched(plain_u)

            def decode(out):
                enc.decode_batched(plain, out)

            def decode_unfused():
                work.copy_(plain)
                enc.plain_nwt_forward_inplace_batched(work)
                torch.index_select(work, 1, imap, out=out_u)

            def run(form):
                if form in ("encode", "encode-kernel"):
                    P.set_batch_encode_path(1 if form == "encode" else 0)
                    enc.encode_batched(values, n, plain if form == "encode" else plain_k)
                elif form == "encode-unfused":
                    encode_unfused()
                elif form == "decode-unfused":
                    decode_unfused()
                else:
                    P.set_batch_decode_path(1 if form == "decode-scatter" else 0)
                    decode(out_s if form == "decode-scatter" else out_g)

            for form in FORMS:                      # fresh buffers: the words agree
                run(form)
            torch.cuda.synchronize()
            same = bool(torch.equal(plain, plain_u) and torch.equal(plain, plain_k) and
                        all(torch.equal(o, values) for o in (out_s, out_g, out_u)))
            for _ in range(3):
                for form in FORMS:
                    run(form)
            times = {form: [] for form in FORMS}
            for _ in range(args.reps):
                for form in FORMS:
                    times[form].append(timed_us(lambda: run(form), args.iters))
            P.set_batch_decode_path(-1)
            P.set_batch_encode_path(-1)
            row = {"log_n": log_n, "t": t, "t_bits": t.bit_length(), "count": count, "same_words": same, "bytes_per_message": 16 * n}
            for form in FORMS:
                med = statistics.median(times[form]) / count
                row[form] = {"us_per_message": med, "min": min(times[form]) / count, "max": max(times[form]) / count,
                             "fraction_of_8TBs": 16 * n / (med * 1e-6) / PEAK}
            rows.append(row)
            print(f"N=2^{log_n} t={t.bit_length()}b count={count:2d} same={same} " +
                  "  ".join(f"{form} {row[form]['us_per_message']:.2f}" for form in FORMS) + "  (us per message)", flush=True)
        del enc, ctx
        torch.cuda.empty_cache()

print("device:", torch.cuda.get_device_name(0))
if args.json:
    with open(args.json, "w") as f:
        json.dump(rows, f, indent=1)
if args.md:
    with open(args.md, "w") as f:
        f.write("| N | t bits | count | " + " | ".join(FORMS) + " | best encode / unfused | best decode / unfused | encode share of 8 TB/s |\n")
        f.write("|---|---|---|" + "---|" * (len(FORMS) + 3) + "\n")
        for r in rows:
            cell = [f"{r[form]['us_per_message']:.2f} ({r[form]['min']:.2f}-{r[form]['max']:.2f})" for form in FORMS]
            best = min(r["decode-scatter"]["us_per_message"], r["decode-gather"]["us_per_message"])
            best_e = min(r["encode"]["us_per_message"], r["encode-kernel"]["us_per_message"])
            f.write(f"| 2^{r['log_n']} | {r['t_bits']} | {r['count']} | " + " | ".join(cell) +
                    f" | {best_e / r['encode-unfused']['us_per_message']:.2f} | "
                    f"{best / r['decode-unfused']['us_per_message']:.2f} | {100 * r['encode']['fraction_of_8TBs']:.2f} % |\n")
