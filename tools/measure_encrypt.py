"""Batched encryption: microseconds per ciphertext of
  entry     pha_encrypt_symmetric_batched / pha_encrypt_asymmetric_batched,
against the loop of the entries the library offered before that computes the same ciphertexts, per ciphertext -- launchers this
change leaves alone -- which is handed the samples already EXPANDED to [rows][N] residues (times t where bgv wants it):
  loop      symmetric, NTT form: pha_nwt_2d_radix8_forward_inplace of the noise residues, pha_multiply_and_add_negate_rns_poly,
            pha_add_rns_poly of the plaintext;
            symmetric, bfv: pha_multiply_rns_poly, pha_nwt_2d_radix8_backward_inplace of c0 and c1, pha_add_and_negate_rns_poly,
            pha_bfv_add_plain;
            asymmetric (top data level: the rows [0, l) u P are all QP rows): forward transform of the residues of u, and per
            polynomial: NTT form the forward transform of the noise residues + pha_multiply_and_add_rns_poly, bfv pha_multiply_rns_poly +
            backward transform + pha_add_rns_poly; pha_moddown per polynomial; the plaintext step.
The loop transforms its residue buffers in place, so from the second call on they hold other (canonical) words: the same work.
The ciphertexts of the two legs are compared once, on fresh buffers, before anything is timed.
Shapes: ckks at c3_ckks16 (N = 2^16, level 45) with count 1, 8, 32; bfv at c4_bfv15 (N = 2^15, level 30) with count 1, 8; symmetric
and asymmetric.  Device events on the launch stream after warm-up, one process, the legs alternating; the median over --reps windows
(default 15) of --iters calls each.  Next to the times the derived global words per word of c0 of the symmetric NTT form: 6 on the
two-pass plans (a, s, plain, the store, the intermediate written and read) against the loop's 12 (the noise residues written by
whoever expands them -- NOT timed here, which favours the loop -- and read, the intermediate written and read, the transform's store,
then a, s, NTT(e) and the store of the product, then c0, plain and the store of the sum) -- counts, not measurements.

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
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--iters", type=int, default=3)
ap.add_argument("--json", default="")
args = ap.parse_args()
sys.path.insert(0, args.pkg)

import torch  # noqa: E402
import phantom_fhe_amd as P  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("measure_encrypt needs a HIP device: there is nothing to time on a CPU")

SETS = [   # scheme, name, log N, bit sizes of QP, special primes, level (the top data level), plain modulus, counts
    ("ckks", "c3_ckks16", 16, [60] + [50] * 44 + [60] * 15, 15, 45, 0, (1, 8, 32)),
    ("bfv", "c4_bfv15", 15, [60] + [50] * 29 + [60] * 15, 15, 30, 65537, (1, 8)),
]
dev = torch.device("cuda:0")


def uniform(shape_front, primes, n, gen):
    d = torch.empty((*shape_front, len(primes), n), dtype=torch.int64, device=dev)
    for i, q in enumerate(primes):
        d[..., i, :] = torch.randint(0, q, (*shape_front, n), dtype=torch.int64, device=dev, generator=gen)
    return d


def residues(v, primes):
    """signed samples [..., N] -> canonical residues [..., len(primes), N]"""
    out = torch.empty((*v.shape[:-1], len(primes), v.shape[-1]), dtype=torch.int64, device=dev)
    for i, q in enumerate(primes):
        out[..., i, :] = torch.remainder(v, q)
    return out


def timed_us(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1000.0 * e0.elapsed_time(e1) / iters


rows = []
for scheme, name, log_n, bits, size_p, level, plain_t, counts in SETS:
    n = 1 << log_n
    primes = [int(p) for p in P.coeff_modulus_create(n, bits)]
    size_qp = len(primes)
    assert level == size_qp - size_p, "the loop below is written for the top data level"
    ctx = P.PhantomContext(log_n, primes, size_p, device=dev)
    kind = P.scheme_type.ckks if scheme == "ckks" else P.scheme_type.bfv
    if plain_t:
        ctx.set_plain_modulus(plain_t)
    gen = torch.Generator(device=dev)
    gen.manual_seed(0xE0C0 + level)
    sk = uniform((), primes, n, gen)
    pk = uniform((2,), primes, n, gen)
    for count in counts:
        a = uniform((count,), primes[:level], n, gen)
        e1 = torch.randint(-21, 22, (count, n), dtype=torch.int64, device=dev, generator=gen)
        e2 = torch.randint(-21, 22, (count, 2, n), dtype=torch.int64, device=dev, generator=gen)
        u = torch.randint(-1, 2, (count, n), dtype=torch.int64, device=dev, generator=gen)
        plain = uniform((count,), primes[:level], n, gen) if scheme == "ckks" else \
            torch.randint(0, plain_t, (count, n), dtype=torch.int64, device=dev, generator=gen)
        for form in ("symmetric", "asymmetric"):
            ct_e = torch.zeros((count, 2, level, n), dtype=torch.int64, device=dev)
            ct_l = torch.zeros((count, 2, level, n), dtype=torch.int64, device=dev)
            if form == "symmetric":
                e_res = residues(e1, primes[:level])

                def fresh():
                    ct_e[:, 1].copy_(a)
                    ct_l[:, 1].copy_(a)
                    e_res.copy_(residues(e1, primes[:level]))

                def entry():
                    ctx.encrypt_symmetric_batched(level, sk, e1, plain, ct_e, kind)

                if scheme == "ckks":
                    def loop():
                        for b in range(count):
                            ctx.nwt_2d_radix8_forward_inplace(e_res[b], level, 0)
                            ctx.multiply_and_add_negate_rns_poly(ct_l[b, 1], sk, e_res[b], ct_l[b, 0], level)
                            ctx.add_rns_poly(ct_l[b, 0], plain[b], ct_l[b, 0], level)
                else:
                    def loop():
                        for b in range(count):
                            ctx.multiply_rns_poly(ct_l[b, 1], sk, ct_l[b, 0], level)
                            ctx.nwt_2d_radix8_backward_inplace(ct_l[b, 0], level, 0)
                            ctx.add_and_negate_rns_poly(ct_l[b, 0], e_res[b], ct_l[b, 0], level)
                            ctx.nwt_2d_radix8_backward_inplace(ct_l[b, 1], level, 0)
                            ctx.bfv_add_plain(level, ct_l[b], plain[b])
            else:
                u_res, e_res = residues(u, primes), residues(e2, primes)
                cx = torch.empty((2, size_qp, n), dtype=torch.int64, device=dev)

                def fresh():
                    u_res.copy_(residues(u, primes))
                    e_res.copy_(residues(e2, primes))

                def entry():
                    ctx.encrypt_asymmetric_batched(level, pk, u, e2, plain, ct_e, kind)

                def loop():
                    for b in range(count):
                        ctx.nwt_2d_radix8_forward_inplace(u_res[b], size_qp, 0)
                        for j in range(2):
                            if scheme == "ckks":
                                ctx.nwt_2d_radix8_forward_inplace(e_res[b, j], size_qp, 0)
                                ctx.multiply_and_add_rns_poly(u_res[b], pk[j], e_res[b, j], cx[j], size_qp)
                            else:
                                ctx.multiply_rns_poly(pk[j], u_res[b], cx[j], size_qp)
                                ctx.nwt_2d_radix8_backward_inplace(cx[j], size_qp, 0)
                                ctx.add_rns_poly(cx[j], e_res[b, j], cx[j], size_qp)
                            ctx.moddown(level, ct_l[b, j], cx[j], kind)
                        if scheme == "ckks":
                            ctx.add_rns_poly(ct_l[b, 0], plain[b], ct_l[b, 0], level)
                        else:
                            ctx.bfv_add_plain(level, ct_l[b], plain[b])

            fresh()
            entry()
            loop()
            torch.cuda.synchronize()
            same = torch.equal(ct_e, ct_l)
            for _ in range(2):
                entry()
                loop()
            te, tl = [], []
            for _ in range(args.reps):
                te.append(timed_us(entry, args.iters))
                tl.append(timed_us(loop, args.iters))
            row = {"scheme": scheme, "set": name, "level": level, "form": form, "count": count, "same_words": bool(same),
                   "entry_us_per_ct": statistics.median(te) / count, "loop_us_per_ct": statistics.median(tl) / count,
                   "entry_min_us": min(te) / count, "loop_min_us": min(tl) / count, "entry_max_us": max(te) / count}
            if form == "symmetric" and scheme == "ckks":
                row["c0_words_entry"], row["c0_words_loop"] = 6, 12
            rows.append(row)
            print(f"{scheme:5s} {name:10s} L={level} {form:10s} count={count:2d}: entry {row['entry_us_per_ct']:9.2f} us/ct  "
                  f"loop {row['loop_us_per_ct']:9.2f} us/ct  ratio {row['loop_us_per_ct'] / row['entry_us_per_ct']:.2f}  same {same}  "
                  f"entry windows {row['entry_min_us']:.2f} .. {row['entry_max_us']:.2f}", flush=True)
            del ct_e, ct_l
    del ctx
    torch.cuda.empty_cache()
print("device:", torch.cuda.get_device_name(0))
if args.json:
    with open(args.json, "w") as f:
        json.dump(rows, f, indent=1)
