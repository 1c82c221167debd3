"""Host compositions of BASELINE.json configurations 4 and 5 over the C-ABI entry points, with the
rank sharding of SURVEY.md 8(e): independent units (ciphertexts / matrix row blocks) are split into contiguous
blocks per rank, every rank runs the same launches on its block, no collective on the data path -- so the
results are bit-identical for every number of ranks.

* config 4: relinearize + Galois rotate of a batch of ciphertexts -- the flows of
  example_bfv_hybrid_key_switching / example_bfv_rotate_row (examples/1_bfv.cu:1269-1336, 1041-1157) at the
  parameter set of benchmark/keyswitch_bench.cu:25-34; relinearize_inplace src/evaluate.cu:1028-1077,
  apply_galois_inplace :1567-1624.
* config 5: encrypted matrix-vector product in diagonal form from hoisted rotations.  The reference has no such
  function (its matmul_bench is a plaintext modular GEMM); the composition is this build's, from the reference's
  hoisting_inplace (src/evaluate.cu:1670-1866), multiply_plain_inplace (:1297-1340) and add_inplace (:116-198).
"""
import hashlib
import os

import numpy as np
import torch

from . import dist as pdist
from .core import scheme_type


def relinearize_rotate_batch(ctx, size_Ql, ct3, relin_key, galois_key, galois_elt, scheme, chunk=0):
    """ct3 [B][3][Ql][N] (a batch of size-3 ciphertexts) -> [B][2][Ql][N]: relinearize, then rotate by
    galois_elt.  BFV ciphertexts are in coefficient form, CKKS / BGV in NTT form, as in the reference.
    One library call (pha_relinearize_rotate_batched): the batch goes through the batched key switches `chunk` ciphertexts
    at a time (0: sized so that the mod-up digits of a set stay within the 256 MiB MALL -- 8 at N = 2^15 / 30 + 15 limbs, where
    that measured fastest), with no copy between the stages."""
    B = ct3.shape[0]
    out = torch.empty_like(ct3[:, :2])
    if B:
        ctx.relinearize_rotate_batched(size_Ql, ct3.contiguous(), B, relin_key.public_keys_ptr, galois_key.public_keys_ptr,
                                       galois_elt, scheme, out, chunk)
    return out


def relinearize_rotate_batch_host(ctx, size_Ql, ct3, relin_key, galois_key, galois_elt, scheme, chunk=8):
    """The same from the two batched key switches and the Galois helper, composed on the host (the r02 form: three
    polynomial copies per ciphertext more); kept as the cross-check of the one-call form."""
    B = ct3.shape[0]
    out = torch.empty_like(ct3[:, :2])
    for b0 in range(0, B, max(1, chunk)):
        out[b0:b0 + chunk] = _relinearize_rotate_chunk(ctx, size_Ql, ct3[b0:b0 + chunk], relin_key, galois_key, galois_elt, scheme)
    return out


def _relinearize_rotate_chunk(ctx, size_Ql, ct3, relin_key, galois_key, galois_elt, scheme):
    B = ct3.shape[0]
    ct = ct3[:, :2].clone(memory_format=torch.contiguous_format)   # never a view: the key switch works in place
    ctx.keyswitch_inplace_batched(size_Ql, ct, ct3[:, 2].contiguous(), B, relin_key.public_keys_ptr, scheme)
    # rotate: (galois(c0), 0) += key switch of galois(c1) (apply_galois_inplace, src/evaluate.cu:1567-1624); one kernel
    # writes both operands in the layout the key switch wants
    rot = torch.empty_like(ct)
    g1 = torch.empty_like(ct[:, 0])
    ctx.apply_galois_for_keyswitch(ct, rot, g1, galois_elt, size_Ql, B, int(scheme) != int(scheme_type.bfv))
    ctx.keyswitch_inplace_batched(size_Ql, rot, g1, B, galois_key.public_keys_ptr, scheme)
    return rot


def relinearize_rotate_sharded(ctx, size_Ql, ct3, relin_key, galois_key, galois_elt, scheme, rank=None, world=None):
    """Config 4 on this rank: the contiguous block shard_range(B, rank, world) of the batch; returns
    (index range, results of that block)."""
    rank = pdist.rank() if rank is None else rank
    world = pdist.world() if world is None else world
    mine = pdist.shard_range(ct3.shape[0], rank, world)
    if len(mine) == 0:
        return mine, ct3[:0, :2].contiguous()
    return mine, relinearize_rotate_batch(ctx, size_Ql, ct3[mine.start:mine.stop], relin_key, galois_key, galois_elt, scheme)


def matrix_diagonals(matrix, slots, steps=None):
    """The generalised diagonals of a d x d matrix (numpy, real or complex; d divides `slots`) as slot vectors: row k is
    diag_k[i] = matrix[i % d][(i + steps[k]) % d] for i < slots, so that sum_k diag_k o rotate_{steps[k]}(v) = matrix v for a vector
    v of period d in the slots (rotate_s(v)[i] = v[i + s]).  steps: the rotation steps (default 0 .. d - 1)."""
    m = np.asarray(matrix, dtype=np.complex128)
    d = m.shape[0]
    if m.ndim != 2 or m.shape[1] != d or d == 0 or slots % d:
        raise ValueError("expected a square matrix whose size divides the slot count")
    steps = list(range(d)) if steps is None else [int(s) for s in steps]
    i = np.arange(slots)
    return np.stack([m[i % d, (i + s) % d] for s in steps])


def encode_diagonals(encoder, size_Ql, matrix, scale, steps=None):
    """The diagonals of `matrix` (matrix_diagonals) encoded on the device as diag_matvec* take them: [len(steps)][Ql + size_P][N]
    in NTT form over the limbs [0, Ql) u P, one batched encode (CKKSEncoder.encode_batched with the special limbs)."""
    ctx = encoder._ctx
    diags = matrix_diagonals(matrix, encoder.slot_count, steps)
    values = torch.from_numpy(np.ascontiguousarray(diags)).to(ctx.device)
    out = torch.empty((diags.shape[0], size_Ql + ctx.size_P, ctx.n), dtype=torch.int64, device=ctx.device)
    encoder.encode_batched(size_Ql, values, encoder.slot_count, scale, out, with_special=True)
    return out


def encode_encrypt_batch(ctx, encoder, messages, level, scale, key, samples, public=False):
    """The entry side of the pipeline, the mirror image of decrypt_decode_batch: messages [B][<= N / 2] complex128 on the device ->
    one batched encode (CKKSEncoder.encode_batched) at `level` data limbs and `scale`, then one batched encryption of the plaintexts
    where the encoder left them; nothing passes through the host.  Returns ckks ciphertexts [B][2][level][N] in NTT form.
    public=False: key = sk_ntt [size_QP][N], samples = (a, e): the uniform a as canonical int64 words, either [B][level][N] (copied
    into c1's place) or the ciphertext buffer itself, [B][2][level][N] with a in [:, 1] (used and returned); e [B][N] signed noise.
    public=True: key = pk [2][size_QP][N] (PhantomContext.public_key_generate), samples = (u, e): u [B][N] ternary, e [B][2][N]."""
    B = messages.shape[0]
    first, e = samples
    if public:
        ct = torch.empty((B, 2, level, ctx.n), dtype=torch.int64, device=ctx.device)
    elif first.dim() == 4:
        ct = first
    else:
        ct = torch.empty((B, 2, level, ctx.n), dtype=torch.int64, device=ctx.device)
        ct[:, 1].copy_(first)
    if B:
        plain = torch.empty((B, level, ctx.n), dtype=torch.int64, device=ctx.device)
        encoder.encode_batched(level, messages, messages.shape[1], scale, plain)
        if public:
            ctx.encrypt_asymmetric_batched(level, key, first, e, plain, ct, scheme_type.ckks)
        else:
            ctx.encrypt_symmetric_batched(level, key, e, plain, ct, scheme_type.ckks)
    return ct


def decrypt_decode_batch(ctx, encoder, cts, level, scale, sk_powers):
    """The exit side of the pipeline for a batch of ckks ciphertexts cts [B][k][level][N] (NTT form, `level` data limbs): the phase
    of every ciphertext under sk_powers (PhantomContext.secret_key_powers) in one launch, then one batched decode
    (CKKSEncoder.decode_batched) at `scale`; the plaintexts stay on the device between the two.  Returns [B][N / 2] complex128."""
    B = cts.shape[0]
    values = torch.empty((B, encoder.slot_count), dtype=torch.complex128, device=ctx.device)
    if B:
        plain = torch.empty((B, level, ctx.n), dtype=torch.int64, device=ctx.device)
        ctx.decrypt_phase_batched(level, cts.contiguous(), sk_powers, plain)
        encoder.decode_batched(level, plain, scale, values)
    return values


def noise_budget_batch(ctx, cts, level, sk_powers, scheme):
    """The invariant noise budget of every ciphertext of cts [B][k][level][N] (bfv: coefficient form, bgv / ckks: NTT form) under
    sk_powers (PhantomContext.secret_key_powers), in bits: int32 [B] on the device, computed there exactly
    (PhantomContext.invariant_noise_budget_batched) -- no host round trip and no synchronisation, so a pipeline can ask after every
    homomorphic step."""
    budget = torch.empty((cts.shape[0],), dtype=torch.int32, device=ctx.device)
    if cts.shape[0]:
        ctx.invariant_noise_budget_batched(level, cts.contiguous(), sk_powers, scheme, budget)
    return budget


def batch_encode_encrypt(ctx, encoder, messages, level, key, samples, scheme, public=False):
    """The bfv / bgv twin of encode_encrypt_batch: messages [B][<= N] int64 words on the device (below t, or negative: the encoder's
    sign rule) -> one batched encode (BatchEncoder.encode_batched), then one batched encryption of the plaintexts [B][N] where the
    encoder left them; nothing passes through the host.  Returns ciphertexts [B][2][level][N], bfv in coefficient form, bgv in NTT form.
    key and samples as encode_encrypt_batch takes them."""
    if int(scheme) not in (int(scheme_type.bfv), int(scheme_type.bgv)):
        raise ValueError("batch_encode_encrypt is for bfv and bgv (ckks: encode_encrypt_batch)")
    B = messages.shape[0]
    first, e = samples
    if public:
        ct = torch.empty((B, 2, level, ctx.n), dtype=torch.int64, device=ctx.device)
    elif first.dim() == 4:
        ct = first
    else:
        ct = torch.empty((B, 2, level, ctx.n), dtype=torch.int64, device=ctx.device)
        ct[:, 1].copy_(first)
    if B:
        plain = torch.empty((B, ctx.n), dtype=torch.int64, device=ctx.device)
        encoder.encode_batched(messages, messages.shape[1], plain)
        if public:
            ctx.encrypt_asymmetric_batched(level, key, first, e, plain, ct, scheme)
        else:
            ctx.encrypt_symmetric_batched(level, key, e, plain, ct, scheme)
    return ct


def batch_decrypt_decode(ctx, encoder, cts, level, sk_powers, scheme, correction_factors=None):
    """The bfv / bgv twin of decrypt_decode_batch for ciphertexts cts [B][k][level][N] (bfv: coefficient form, bgv: NTT form): one
    batched decryption (bfv_decrypt_batched / bgv_decrypt_batched; correction_factors: bgv only) into plaintexts [B][N], then one
    batched decode (BatchEncoder.decode_batched); the plaintexts stay on the device between the two.  Returns [B][N] int64 words
    below t."""
    if int(scheme) not in (int(scheme_type.bfv), int(scheme_type.bgv)):
        raise ValueError("batch_decrypt_decode is for bfv and bgv (ckks: decrypt_decode_batch)")
    B = cts.shape[0]
    values = torch.empty((B, encoder.slot_count), dtype=torch.int64, device=ctx.device)
    if B:
        plain = torch.empty((B, ctx.n), dtype=torch.int64, device=ctx.device)
        if int(scheme) == int(scheme_type.bfv):
            ctx.bfv_decrypt_batched(level, cts.contiguous(), sk_powers, plain)
        else:
            ctx.bgv_decrypt_batched(level, cts.contiguous(), sk_powers, plain, correction_factors)
        encoder.decode_batched(plain, values)
    return values


def derive_seeds(master, label, count):
    """`count` 64-byte child seeds of `master` (bytes; None: os.urandom(64)) as a uint8 numpy array [count][64], on the host:
    seed i = blake2b(master || label || i as 8 little-endian bytes, digest_size=64).  Different labels and different counters give
    unrelated seeds; the same (master, label, i) always gives the same one."""
    master = os.urandom(64) if master is None else bytes(master)
    label = label.encode() if isinstance(label, str) else bytes(label)
    out = np.empty((int(count), 64), dtype=np.uint8)
    for i in range(int(count)):
        out[i] = np.frombuffer(hashlib.blake2b(master + label + i.to_bytes(8, "little"), digest_size=64).digest(), dtype=np.uint8)
    return out


def _device_seeds(ctx, master, label, count):
    return torch.from_numpy(derive_seeds(master, label, count)).to(ctx.device)


def keygen(ctx, scheme, galois_elts=(), master=None, max_power=2):
    """Every key of one party from one master seed (None: fresh entropy), sampled and built on the device: a dict with
    sk_ntt [size_QP][N] (gen_secretkey), sk_powers [max_power][size_QP][N] (compute_secret_key_array), pk [2][size_QP][N]
    (gen_publickey), relin (PhantomRelinKey of s^2: gen_relinkey), galois ({element: PhantomRelinKey}: create_galois_keys) and the
    master seed used.  The only host work is the derivation of the 64-byte seeds (derive_seeds, labels "sk", "pk", "ksk")."""
    master = os.urandom(64) if master is None else bytes(master)
    elts = [int(e) for e in galois_elts]
    dnum = ctx.size_Q // ctx.size_P
    sk_ntt = ctx.secret_key_generate(_device_seeds(ctx, master, "sk", 1))
    sk_powers = ctx.secret_key_powers(sk_ntt, max(int(max_power), 2))
    pk_seeds = _device_seeds(ctx, master, "pk", 2)                       # the uniform seed, the noise seed
    pk = torch.empty((2, ctx.size_QP, ctx.n), dtype=torch.int64, device=ctx.device)
    e = torch.empty((1, ctx.n), dtype=torch.int64, device=ctx.device)
    ctx.sample_uniform_batched(ctx.size_Q, pk_seeds[0:1], pk[1:2], with_special=True)
    ctx.sample_error_signed_batched(pk_seeds[1:2], e)
    ctx.public_key_generate(sk_ntt, e, pk, scheme)
    # key 0 switches from s^2, key 1 + i from galois_elts[i] (s)
    new_keys = torch.empty((1 + len(elts), ctx.size_Q, ctx.n), dtype=torch.int64, device=ctx.device)
    new_keys[0].copy_(sk_powers[1, :ctx.size_Q])
    for i, elt in enumerate(elts):
        ctx.apply_galois_ntt(sk_ntt, new_keys[1 + i], elt, ctx.size_Q)
    keys = ctx.generate_kswitch_keys_seeded(sk_ntt, new_keys, _device_seeds(ctx, master, "ksk", 2 * dnum * (1 + len(elts))), scheme)
    return {"sk_ntt": sk_ntt, "sk_powers": sk_powers, "pk": pk, "relin": keys[0], "galois": dict(zip(elts, keys[1:])), "master": master}


def sample_encryption(ctx, level, count, master, public=False):
    """The `samples` tuple encode_encrypt_batch / batch_encode_encrypt take for `count` ciphertexts at `level` data limbs, sampled on
    the device from seeds derived from `master` (labels "enc.a" / "enc.e", "enc.u").  public=False: (ct, e) with ct the ciphertext
    buffer [count][2][level][N] whose [:, 1] holds the uniform a (sampled in place, never copied) and e [count][N];
    public=True: (u, e) with u [count][N] ternary and e [count][2][N], one seed per polynomial."""
    n = ctx.n
    if public:
        u = torch.empty((count, n), dtype=torch.int64, device=ctx.device)
        e = torch.empty((count, 2, n), dtype=torch.int64, device=ctx.device)
        if count:
            ctx.sample_ternary_signed_batched(_device_seeds(ctx, master, "enc.u", count), u)
            ctx.sample_error_signed_batched(_device_seeds(ctx, master, "enc.e", 2 * count), e.view(2 * count, n))
        return u, e
    ct = torch.empty((count, 2, level, n), dtype=torch.int64, device=ctx.device)
    e = torch.empty((count, n), dtype=torch.int64, device=ctx.device)
    if count:
        ctx.sample_uniform_batched(level, _device_seeds(ctx, master, "enc.a", count), ct[:, 1])
        ctx.sample_error_signed_batched(_device_seeds(ctx, master, "enc.e", count), e)
    return ct, e


def diag_matvec(ctx, size_Ql, ct, galois_elts, galois_keys, diagonals, scheme):
    """One block of config 5: out = sum_k diagonals[k] (.) rotate_{galois_elts[k]}(ct) (Halevi-Shoup diagonal
    form), all rotations hoisted behind one mod-up and one mod-down (pha_hoisting_weighted).  diagonals[k] is the
    k-th generalised diagonal encoded over [Q_l || P] in NTT form, [Ql + size_P][N]; Galois element 1 (the main
    diagonal) takes no key."""
    out = ct.clone()
    ctx.hoisting_weighted(size_Ql, out, galois_elts, galois_keys, diagonals, scheme)
    return out


def diag_matvec_batch(ctx, size_Ql, cts, galois_elts, galois_keys, diagonals, scheme, chunk=0):
    """The same block applied to a batch of encrypted vectors cts [B][2][Ql][N] (pha_hoisting_weighted_batched): the Galois keys and
    the diagonals are read once per group of ciphertexts instead of once per vector.  `chunk` vectors go through one set of
    launches (0: the library's default).  Returns [B][2][Ql][N]; every result equals diag_matvec of that vector."""
    return ctx.hoisting_weighted_batched(size_Ql, cts, galois_elts, galois_keys, diagonals, scheme, chunk=chunk)


def diag_matvec_bsgs(ctx, size_Ql, ct, baby_elts, baby_keys, giant_elts, giant_keys, diagonals, scheme):
    """The same block in baby-step / giant-step form (pha_hoisting_weighted_bsgs): with d = n_giant * n_baby diagonals,
    out = sum_i rot_{giant_elts[i]}(sum_j diagonals[i][j] (.) rot_{baby_elts[j]}(ct)) from n_baby + n_giant - 2 Galois keys instead of
    d - 1.  diagonals[i][j] is diagonal i * n_baby + j of the matrix (matrix_diagonals), rotated back by giant step i -- rotate_{-g} with
    g = i * n_baby the step of giant_elts[i], np.roll(diag, +g) on the slot vector -- and encoded over [Q_l || P] ([Ql + size_P][N], NTT
    form): the usual offline preparation of the BSGS matrix-vector product (tests/ckks_semantics.py: bsgs_diagonals)."""
    out = ct.clone()
    ctx.hoisting_weighted_bsgs(size_Ql, out, baby_elts, baby_keys, giant_elts, giant_keys, diagonals, scheme)
    return out


def diag_matvec_bsgs_batch(ctx, size_Ql, cts, baby_elts, baby_keys, giant_elts, giant_keys, diagonals, scheme, chunk=0):
    """The baby-step / giant-step block applied to a batch of encrypted vectors cts [B][2][Ql][N]
    (pha_hoisting_weighted_bsgs_batched): the baby keys and the diagonals are read once per group of ciphertexts instead of once per
    vector.  `chunk` vectors go through one set of launches (0: the library's default).  Returns [B][2][Ql][N]; every result equals
    diag_matvec_bsgs of that vector."""
    return ctx.hoisting_weighted_bsgs_batched(size_Ql, cts, baby_elts, baby_keys, giant_elts, giant_keys, diagonals, scheme, chunk=chunk)


def diag_matvec_bsgs_blocks(ctx, size_Ql, ct, baby_elts, baby_keys, giant_elts, giant_keys, blocks, scheme, per_call=0):
    """Several row blocks of the matrix against ONE encrypted vector (pha_hoisting_weighted_bsgs_blocks): blocks[r][i][j] as in
    diag_matvec_bsgs.  `per_call` blocks go through one call (0: as many as make 16 (block, giant step) accumulators, the width of
    the fused baby-step kernel, so that the baby keys are streamed once per that many blocks).  Returns [len(blocks)][2][Ql][N];
    every block equals its own diag_matvec_bsgs."""
    import torch
    nblk = len(blocks)
    out = torch.empty((nblk,) + tuple(ct.shape), dtype=ct.dtype, device=ct.device)
    if per_call <= 0:
        per_call = max(1, 16 // max(1, len(giant_elts)))
    for r0 in range(0, nblk, per_call):
        ctx.hoisting_weighted_bsgs_blocks(size_Ql, ct, baby_elts, baby_keys, giant_elts, giant_keys, blocks[r0:r0 + per_call],
                                          out[r0:r0 + per_call], scheme)
    return out


def matvec_row_blocks_sharded(ctx, size_Ql, ct, galois_elts, galois_keys, blocks, scheme, rank=None, world=None):
    """Config 5 on this rank: `blocks` is a list of row blocks of the matrix, each a list of encoded diagonals
    (one output ciphertext per block); blocks are split contiguously over the ranks.  Returns (index range,
    list of output ciphertexts of that range)."""
    rank = pdist.rank() if rank is None else rank
    world = pdist.world() if world is None else world
    mine = pdist.shard_range(len(blocks), rank, world)
    return mine, [diag_matvec(ctx, size_Ql, ct, galois_elts, galois_keys, blocks[i], scheme) for i in mine]
