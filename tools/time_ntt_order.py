"""Same-session A/B of the block order of the batched NTT launch pair (csrc/pha_ntt.hip: -DPHA_NTT_PASS_ORDER=0 the plain grid of the
strided pass, 1 the reverse of the contiguous pass's order, 2 the same in two limb-range halves per launch).  Builds:

  tools/build_variant.sh order0 -DPHA_NTT_PASS_ORDER=0      (likewise order1, order2; order1t, the integer limbs at the tail of the
                                                             strided launch: "-DPHA_NTT_PASS_ORDER=1 -DPHA_NTT_ORDER_INT_HEAD=0")

Every measurement runs in a process of its own (PHA_LIB_OVERRIDE is per process) under its own `timeout`; the builds alternate
--rounds times (default 5), so that each build's repeats are spread over the session.  A build's process reports ms per step for
  (a) fwd16 / fwd8   back-to-back forward steps of 16 x 45 and 8 x 45 limbs at N = 2^16 through repeat_forward_ntt_batched, as
                     bench.py times them (warm-up, 0.2 s clock ramp, then windows of 100 steps; the median window);
  (b) inv16 / inv8   back-to-back inverse steps, likewise (enqueued call by call);
  (c) cold_fwd16 / cold_inv16   single calls, each after a 512 MiB read-modify-write stream that empties the last-level cache: what the
                     order gains inside one call (the intermediate's reads) apart from what it gains from step to step;
and a checksum of one forward and one inverse transform of seeded inputs, which must agree between the builds.

The table gives, per build and protocol, the median, minimum and maximum of its repeats, the gain of each build over the FIRST build
listed, and that first build's own range (max - min): a gain counts only where it is larger than that range.

  --builds order0,order1,order2   names of libphantom_amd_NAME.so in the package directory (`product` = libphantom_amd.so); the first is the baseline
  --rounds R                      alternations (default 5)
  --timeout S                     seconds per process (default 240)
  --one BUILD:PROTOCOL            ten warm-up steps and 50 steps of that protocol, nothing else: run it under
                                  `rocprofv3 --kernel-trace --stats` for the two passes' kernel times (in this process; PHA_LIB_OVERRIDE
                                  is set from BUILD before the library loads)
  --json PATH                     also write everything as JSON
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "phantom-fhe_amd")
ap = argparse.ArgumentParser()
ap.add_argument("--builds", default="order0,order1,order2")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--timeout", type=int, default=240)
ap.add_argument("--one", default="")
ap.add_argument("--json", default="")
ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
args = ap.parse_args()

PROTOCOLS = ["fwd16", "fwd8", "inv16", "inv8", "cold_fwd16", "cold_inv16"]
LOG_N, BITS, SIZE_P, QL = 16, [60] + [50] * 44 + [60] * 15, 15, 45
WINDOW, WINDOWS, COLD_CALLS, FLUSH_BYTES = 100, 5, 20, 512 << 20


def lib_of(name):
    return os.path.join(PKG, "phantom_fhe_amd", "libphantom_amd.so" if name == "product" else f"libphantom_amd_{name}.so")


def measure(one=""):
    """Runs in the process whose library is already chosen.  Returns {protocol: ms, "chk_fwd": .., "chk_inv": ..}."""
    import time
    sys.path.insert(0, PKG)
    import torch
    import phantom_fhe_amd as P
    if not torch.cuda.is_available():
        sys.exit("time_ntt_order needs a HIP device: there is nothing to time on a CPU")
    dev = torch.device("cuda:0")
    n = 1 << LOG_N
    primes = [int(p) for p in P.coeff_modulus_create(n, BITS)]
    ctx = P.PhantomContext(LOG_N, primes, SIZE_P, device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(45)
    polys = torch.empty((16, QL, n), dtype=torch.int64, device=dev)
    for i, q in enumerate(primes[:QL]):
        polys[:, i] = torch.randint(0, q, (16, n), dtype=torch.int64, device=dev, generator=gen)
    seeded = polys.clone()
    stride = QL * n
    flush = torch.zeros(FLUSH_BYTES // 8, dtype=torch.int64, device=dev)

    def fwd(nb, reps):
        ctx.repeat_forward_ntt_batched(polys, QL, 0, nb, stride, reps)

    def inv(nb, reps):
        for _ in range(reps):
            ctx.nwt_2d_radix8_backward_inplace_batched(polys, QL, 0, nb, stride)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def back_to_back(step, nb):
        step(nb, 10)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.2:        # clock ramp, as bench.py
            step(nb, 10)
            torch.cuda.synchronize()
        return statistics.median(timed(lambda: step(nb, WINDOW)) / WINDOW for _ in range(WINDOWS))

    def cold(step):
        step(16, 3)
        ms = []
        for _ in range(COLD_CALLS):
            flush.add_(1)
            ms.append(timed(lambda: step(16, 1)))
        return statistics.median(ms)

    runs = {"fwd16": lambda: back_to_back(fwd, 16), "fwd8": lambda: back_to_back(fwd, 8), "inv16": lambda: back_to_back(inv, 16),
            "inv8": lambda: back_to_back(inv, 8), "cold_fwd16": lambda: cold(fwd), "cold_inv16": lambda: cold(inv)}
    if one:
        step, nb = (fwd if "fwd" in one else inv), (8 if one.endswith("8") else 16)
        step(nb, 10)
        torch.cuda.synchronize()
        step(nb, 50)
        torch.cuda.synchronize()
        print(f"ten warm-up steps and 50 steps of {one}")
        return {}
    out = {}
    polys.copy_(seeded)
    fwd(16, 1)
    out["chk_fwd"] = f"{int(polys.sum().item()) & 0xffffffffffffffff:016x}"
    polys.copy_(seeded)
    inv(16, 1)
    out["chk_inv"] = f"{int(polys.sum().item()) & 0xffffffffffffffff:016x}"
    for name in PROTOCOLS:
        out[name] = runs[name]()
    out["device"] = torch.cuda.get_device_name(0)
    return out


if args.child:
    print("RESULT " + json.dumps(measure()), flush=True)
    sys.exit(0)
if args.one:
    build, protocol = args.one.split(":", 1)
    if protocol not in PROTOCOLS[:4]:
        sys.exit("--one takes BUILD:fwd16, fwd8, inv16 or inv8")
    os.environ["PHA_LIB_OVERRIDE"] = lib_of(build)
    measure(protocol)
    sys.exit(0)

builds = args.builds.split(",")
for b in builds:
    if not os.path.exists(lib_of(b)):
        sys.exit(f"{lib_of(b)} is missing: tools/build_variant.sh {b} -DPHA_NTT_PASS_ORDER=...")
results = {b: [] for b in builds}
for rnd in range(args.rounds):
    for b in builds:
        env = dict(os.environ, PHA_LIB_OVERRIDE=lib_of(b))
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child"]
        p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not line:   # a fault, an abort or the time limit: nothing more runs on the device
            sys.stdout.write(p.stdout)
            sys.exit(f"round {rnd}, build {b}: exit status {p.returncode}; stopping")
        r = json.loads(line[0][len("RESULT "):])
        results[b].append(r)
        print(f"round {rnd} {b:8s} " + " ".join(f"{k} {r[k]:.4f}" for k in PROTOCOLS) + f"  chk {r['chk_fwd']} {r['chk_inv']}", flush=True)

chks = {(r["chk_fwd"], r["chk_inv"]) for b in builds for r in results[b]}
if len(chks) != 1:
    sys.exit(f"the builds' outputs differ: {sorted(chks)}")
print(f"\nchecksums agree over {len(builds)} builds x {args.rounds} rounds: forward {results[builds[0]][0]['chk_fwd']}, inverse {results[builds[0]][0]['chk_inv']}")
print(f"device: {results[builds[0]][0]['device']}; ms per step, median [min .. max] of {args.rounds} repeats; gain over {builds[0]} "
      f"(counts where it exceeds that build's own range)\n")
summary = {}
for k in PROTOCOLS:
    base = [r[k] for r in results[builds[0]]]
    base_med, base_range = statistics.median(base), max(base) - min(base)
    for b in builds:
        v = [r[k] for r in results[b]]
        med = statistics.median(v)
        gain = base_med - med
        row = {"median_ms": med, "min_ms": min(v), "max_ms": max(v), "gain_ms": gain, "gain_pct": 100.0 * gain / base_med,
               "baseline_range_ms": base_range, "beyond_noise": b != builds[0] and abs(gain) > base_range}
        summary.setdefault(k, {})[b] = row
        tail = "" if b == builds[0] else (f"  gain {1e3 * gain:+7.1f} us ({row['gain_pct']:+5.2f} %) vs range {1e3 * base_range:5.1f} us: "
                                           + ("faster" if gain > base_range else "slower" if -gain > base_range else "within noise"))
        print(f"{k:11s} {b:8s} {med:.4f} [{min(v):.4f} .. {max(v):.4f}]{tail}")
    print()
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump({"tool": "time_ntt_order", "builds": builds, "rounds": args.rounds, "results": results, "summary": summary}, f, indent=1)
