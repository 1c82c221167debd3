"""CKKS encoder at configuration 3 (N = 2^16, 45 data limbs + 15 special): milliseconds per call of
  encode  pha_ckks_encode_batched for count = 1, 8, 128 messages of N / 2 values, at size_Ql = 45 with the special limbs (the layout
          the hoisting entries take: 60 limbs) and at size_Ql = 3, on the path the library's rule picks,
  fused / unfused  the same call with the path forced (pha_ckks_set_encode_path): round-and-reduce as the load prologue of the forward
          transform's first pass, against the decompose kernel followed by the plain transform,
  floor   the bare batched forward transform of the same number of limbs and polynomials (pha_nwt_2d_radix8_forward_inplace_batched,
          unchanged by the encoder), which every encoding ends with,
  decode  pha_ckks_decode_batched at size_Ql = 2 and 45.
Device events on the launch stream after warm-up, one process, the legs alternating; median, minimum and spread over the windows.
encode synchronises the stream once per call (it reads the maxima back), so its time includes that round trip.  Also encode's
achieved bytes/s over its algorithmic bytes -- 16 n for the values, 8 N for the coefficients written and 8 N read back (in cache for
all limbs but the first), the hand-over of the two-pass FFT 2 * 16 n, and for the limbs 3 * 8 L N fused (the first pass writes, the
second reads and writes) or 5 * 8 L N unfused (the decomposed form written and read as well; `encode` is counted as fused) -- and the
fraction of the 8 TB/s HBM peak.

  --counts 1,8,128    messages per call
  --reps R            windows per leg (default 7)
  --json PATH         also write the rows as JSON
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--pkg", default=os.path.join(ROOT, "phantom-fhe_amd"))
ap.add_argument("--counts", default="1,8,128")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--json", default="")
args = ap.parse_args()
sys.path.insert(0, args.pkg)

import torch  # noqa: E402
import phantom_fhe_amd as P  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("time_ckks_encoder needs a HIP device: there is nothing to time on a CPU")

PEAK_HBM = 8.0e12
LOG_N, BITS, SIZE_P = 16, [60] + [50] * 44 + [60] * 15, 15
SCALE = 2.0 ** 40
dev = torch.device("cuda:0")
n_coeff = 1 << LOG_N
slots = n_coeff // 2
primes = [int(p) for p in P.coeff_modulus_create(n_coeff, BITS)]
ctx = P.PhantomContext(LOG_N, primes, SIZE_P, device=dev)
enc = ctx.ckks_encoder()
size_q = len(primes) - SIZE_P


def timed_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def encode_bytes(count, limbs, fused=True):
    """Every global read and write, cached or not: values, coefficients written and read, the two-pass FFT's hand-over, and the limb
    words -- fused 3 L N (first pass writes, second reads and writes), unfused 5 L N (the decomposed form written and read as well)."""
    return count * (16.0 * slots + 16.0 * n_coeff + 32.0 * slots + (24.0 if fused else 40.0) * limbs * n_coeff)


def measure(tag, legs, reps, extra=None):
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
        r = {"shape": tag, "leg": name, "ms_median": round(med, 5), "ms_min": round(lo, 5), "ms_max": round(hi, 5),
             "spread_pct": round(100.0 * (hi - lo) / med, 2), "windows": len(ms[name]), "iters_per_window": iters[name]}
        if extra and name in extra:
            rate = extra[name] / (med * 1e-3)
            r.update(algorithmic_MB=round(extra[name] / 1e6, 1), TB_per_s=round(rate / 1e12, 3), frac_of_8TBs=round(rate / PEAK_HBM, 4))
        rows.append(r)
        more = f"  {r['algorithmic_MB']:.0f} MB, {r['TB_per_s']:.3f} TB/s = {r['frac_of_8TBs']:.3f} of 8 TB/s" if "TB_per_s" in r else ""
        print(f"{tag} {name:7s} {med:9.4f} ms (min {lo:.4f}, max {hi:.4f}, spread {r['spread_pct']:.1f} %){more}", flush=True)
    return rows


rows = []
gen = torch.Generator(device=dev)
gen.manual_seed(7)
for count in [int(c) for c in args.counts.split(",")]:
    values = torch.complex(*(torch.rand((2, count, slots), dtype=torch.float64, device=dev, generator=gen) * 2 - 1))
    for size_Ql, special in ((size_q, True), (3, False)):
        limbs = size_Ql + (SIZE_P if special else 0)
        dst = torch.empty((count, limbs, n_coeff), dtype=torch.int64, device=dev)
        work = torch.zeros((count, limbs, n_coeff), dtype=torch.int64, device=dev)   # canonical words for the bare transform
        def path_leg(mode):
            def leg():
                P.set_ckks_encode_path(mode)
                enc.encode_batched(size_Ql, values, slots, SCALE, dst, with_special=special)
            return leg

        P.set_ckks_encode_path(-1)
        legs = [("encode", path_leg(-1)),
                ("fused", path_leg(1)), ("unfused", path_leg(0)),
                ("floor", lambda: ctx.nwt_2d_radix8_forward_inplace_batched(work, limbs, 0, count, limbs * n_coeff))]
        got = measure(f"count={count:<3d} Ql={size_Ql:<2d} special={int(special)}", legs, args.reps,
                      {"encode": encode_bytes(count, limbs), "fused": encode_bytes(count, limbs, True), "unfused": encode_bytes(count, limbs, False)})
        P.set_ckks_encode_path(-1)
        by = {r["leg"]: r for r in got}
        ratio = round(by["encode"]["ms_median"] / by["floor"]["ms_median"], 3)
        uf = round(by["unfused"]["ms_median"] / by["fused"]["ms_median"], 3)
        print(f"    encode / floor = {ratio}   unfused / fused = {uf} (beyond spread: "
              f"{by['fused']['ms_max'] < by['unfused']['ms_min'] or by['unfused']['ms_max'] < by['fused']['ms_min']})", flush=True)
        rows += got + [{"shape": got[0]["shape"], "leg": "ratios", "encode_over_floor": ratio, "unfused_over_fused": uf}]
        del dst, work
        torch.cuda.empty_cache()
    if count <= 8:
        for size_Ql in (2, size_q):
            plain = torch.empty((count, size_Ql, n_coeff), dtype=torch.int64, device=dev)
            enc.encode_batched(size_Ql, values, slots, SCALE, plain)
            out = torch.empty((count, slots), dtype=torch.complex128, device=dev)
            rows += measure(f"count={count:<3d} Ql={size_Ql:<2d} decode   ", [("decode", lambda: enc.decode_batched(size_Ql, plain, SCALE, out))],
                            args.reps)
            del plain, out
            torch.cuda.empty_cache()

out = {"tool": "time_ckks_encoder", "device": torch.cuda.get_device_name(0), "rows": rows}
print(json.dumps(out))
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
