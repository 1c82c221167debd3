"""Seeded samplers and seeded key generation at c3_ckks16 (N = 2^16, 45 + 15 limbs, dnum 3), the key level:
  (i)   pha_sample_uniform_batched over all 60 QP rows: one key component (60 * 65536 words) and 16 * 3 components in one call, in
        words and bytes written per second, next to the issue bound derived from the instruction count of the ISA (DESIGN.md 4.14:
        about 1150 vector instructions per 64-byte block and lane, 16384 lane-instructions per cycle, 1.9 .. 2.4 GHz);
  (ii)  pha_generate_kswitch_keys_seeded for 1 and 16 keys against the route the library offered before to the same kind of keys:
        numpy-made a and e EXPANDED to [dnum][QP][N] residues on the host, the host-to-device copy of both, and
        pha_generate_one_kswitch_key per key.  The copy (wall clock around a synchronised copy from pageable host memory) and the
        arithmetic (device events) are timed separately; making the numbers on the host is not timed at all;
  (iii) the noise sampler in the compact [N] signed form against the reference layout ([60][N] residues).
Device events on the launch stream after warm-up, one process; the median over --reps windows (default 9) of --iters calls each.
The seeded keys are compared with pha_generate_one_kswitch_key on the sampler's own a and e once, before anything is timed.

  --out PATH    write the table as markdown (default: standard output only)
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--pkg", default=os.path.join(ROOT, "phantom-fhe_amd"))
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--iters", type=int, default=3)
ap.add_argument("--out", default="")
args = ap.parse_args()
sys.path.insert(0, args.pkg)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import phantom_fhe_amd as P  # noqa: E402
from phantom_fhe_amd import lib as L  # noqa: E402
from phantom_fhe_amd import workloads as W  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("measure_prng needs a HIP device: there is nothing to time on a CPU")

LOG_N, BITS, SIZE_P = 16, [60] + [50] * 44 + [60] * 15, 15
N, QP, Q = 1 << LOG_N, len(BITS), len(BITS) - SIZE_P
DNUM = Q // SIZE_P
INSTR_PER_BLOCK, LANES_PER_CYCLE, CLOCKS = 1150, 16384, (1.9e9, 2.4e9)
dev = torch.device("cuda:0")
primes = [int(q) for q in P.coeff_modulus_create(N, BITS)]
ctx = P.PhantomContext(LOG_N, primes, SIZE_P, device=dev)
kind = P.scheme_type.ckks
MASTER = bytes(range(64))


def seeds(label, count):
    return torch.from_numpy(W.derive_seeds(MASTER, label, count)).to(dev)


legs = []   # the windows of every timed leg, in the order of the calls


def timed(fn):
    """Median microseconds per call: windows of --iters calls between device events, after two warm-up calls."""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.iters):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1000.0 / args.iters)
    print(f"windows of timed leg {len(legs)}: median {statistics.median(out):.2f} min {min(out):.2f} max {max(out):.2f} us", flush=True)
    legs.append(out)
    return statistics.median(out)


rows = []

# ---- (i) the uniform sampler ----------------------------------------------------------------------------------------------------
for comps in (1, 16 * DNUM):
    buf = torch.empty((comps, 2, QP, N), dtype=torch.int64, device=dev)
    sd = seeds("measure.a", comps)
    us = timed(lambda: ctx.sample_uniform_batched(Q, sd, buf[:, 1], with_special=True))
    words = comps * QP * N
    rows.append(("i", f"uniform sampler, {comps} component(s) of [60][N]", f"{us:.1f} us", f"{words / us * 1e6:.3e} words/s = {words * 8 / us / 1e6:.2f} TB/s written"))
    del buf
bound = [LANES_PER_CYCLE * c / INSTR_PER_BLOCK * 64 / 1e12 for c in CLOCKS]
rows.append(("i", f"issue bound, derived: {INSTR_PER_BLOCK} vector instructions per 64-byte block (ISA), {LANES_PER_CYCLE} lane-instructions per cycle",
             "-", f"{bound[0]:.2f} .. {bound[1]:.2f} TB/s at 1.9 .. 2.4 GHz"))
torch.cuda.empty_cache()

# ---- (ii) key generation ------------------------------------------------------------------------------------------------------------
sk = ctx.secret_key_generate(seeds("measure.sk", 1))
rng = np.random.default_rng(5)
host_a = np.stack([np.stack([rng.integers(0, q, N, dtype=np.uint64) for q in primes]) for _ in range(DNUM)])
small = rng.integers(-21, 22, (DNUM, N))
host_e = np.stack([np.stack([(small[d] % q).astype(np.uint64) for q in primes]) for d in range(DNUM)])
for n_keys in (1, 16):
    new_keys = torch.randint(0, 1 << 40, (n_keys, Q, N), dtype=torch.int64, device=dev)
    sd = seeds("measure.ksk", 2 * n_keys * DNUM)
    evk = torch.empty((n_keys, DNUM, 2, QP, N), dtype=torch.int64, device=dev)
    keys = ctx.generate_kswitch_keys_seeded(sk, new_keys, sd, kind, evk=evk)
    if n_keys == 1:   # the same words as the entry of before on the sampler's own a and e
        a = evk[0, :, 1].contiguous()
        e_signed = torch.empty((DNUM, N), dtype=torch.int64, device=dev)
        ctx.sample_error_signed_batched(sd.view(DNUM, 2, 64)[:, 1].contiguous(), e_signed)
        q_col = torch.tensor(primes, dtype=torch.int64, device=dev).view(1, QP, 1)
        e = torch.where(e_signed.view(DNUM, 1, N) < 0, e_signed.view(DNUM, 1, N) + q_col, e_signed.view(DNUM, 1, N).expand(DNUM, QP, N)).contiguous()
        ref = ctx.generate_one_kswitch_key(sk, new_keys[0], a, e, kind)
        assert all(torch.equal(ref.public_keys[d], evk[0, d]) for d in range(DNUM)), "seeded keys differ from pha_generate_one_kswitch_key"
    st = torch.cuda.current_stream().cuda_stream      # the timed legs call the library directly: no table of pointers is rebuilt per call

    def seeded():
        L.check(ctx._L.pha_generate_kswitch_keys_seeded(ctx._h, sk.data_ptr(), new_keys.data_ptr(), n_keys, Q * N, sd.data_ptr(), evk.data_ptr(),
                                                        2 * QP * N, int(kind), st))
    us = timed(seeded)
    rows.append(("ii", f"pha_generate_kswitch_keys_seeded, {n_keys} key(s)", f"{us:.1f} us", f"{us / n_keys:.1f} us per key"))
    # the route of before: copy a and e (pageable host memory, as numpy makes them), then one call per key
    d_a = torch.empty((DNUM, QP, N), dtype=torch.int64, device=dev)
    d_e = torch.empty((DNUM, QP, N), dtype=torch.int64, device=dev)
    t_a, t_e = torch.from_numpy(host_a.view(np.int64)), torch.from_numpy(host_e.view(np.int64))
    copies = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n_keys):
            d_a.copy_(t_a)
            d_e.copy_(t_e)
        torch.cuda.synchronize()
        copies.append((time.perf_counter() - t0) * 1e6)
    copy_us = statistics.median(copies)

    def before():
        for k in range(n_keys):   # (e is transformed in place: other canonical words, the same work)
            L.check(ctx._L.pha_generate_one_kswitch_key(ctx._h, sk.data_ptr(), new_keys[k].data_ptr(), d_a.data_ptr(), d_e.data_ptr(),
                                                        keys[k].public_keys_ptr.data_ptr(), int(kind), st))
    arith_us = timed(before)
    mb = n_keys * 2 * DNUM * QP * N * 8 / 1e6
    rows.append(("ii", f"before, {n_keys} key(s): host-to-device copy of a and expanded e ({mb:.0f} MB)", f"{copy_us:.0f} us", f"{mb / copy_us * 1e6 / 1e3:.1f} GB/s"))
    rows.append(("ii", f"before, {n_keys} key(s): pha_generate_one_kswitch_key per key",
                 f"{arith_us:.1f} us", f"copy + arithmetic = {copy_us + arith_us:.0f} us = {(copy_us + arith_us) / us:.1f} x the seeded call"))
    del evk, keys, new_keys, d_a, d_e
    torch.cuda.empty_cache()

# ---- (iii) the noise sampler, compact against the reference layout -------------------------------------------------------------------
sd = seeds("measure.e", 1)
compact = torch.empty((1, N), dtype=torch.int64, device=dev)
full = torch.empty((QP, N), dtype=torch.int64, device=dev)
us_c = timed(lambda: ctx.sample_error_signed_batched(sd, compact))
us_f = timed(lambda: ctx.sample_error_poly(full, sd, QP, 0))
rows.append(("iii", "noise, compact [N] signed words", f"{us_c:.1f} us", f"{N * 8 / 1e6:.2f} MB written"))
rows.append(("iii", "noise, reference layout [60][N] residues (one block per coefficient, 60 stores)", f"{us_f:.1f} us",
             f"{QP * N * 8 / 1e6:.1f} MB written; {us_f / us_c:.1f} x the compact form"))

text = "| | what | median | derived |\n|---|---|---|---|\n" + "\n".join(f"| {a} | {b} | {c} | {d} |" for a, b, c, d in rows) + "\n"
print(f"device: {torch.cuda.get_device_name(0)}; reps {args.reps}, iters {args.iters}\n")
print(text)
if args.out:
    with open(args.out, "w") as f:
        f.write(f"device: {torch.cuda.get_device_name(0)}; reps {args.reps}, iters {args.iters}\n\n" + text)
