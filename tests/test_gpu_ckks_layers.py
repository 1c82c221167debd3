"""The upper layers of the CKKS encoder on the GPU: PhantomCKKSEncoder (host/phantom.h) through pyPhantom.ckks_encoder gives the
words and doubles of the C entries (pha_ckks_encode_batched / pha_ckks_decode_batched through the ctypes layer, themselves compared
with the restatement in tests/test_gpu_ckks_encoder.py); the calls of the reference's python/examples/ckks.py resolve;
workloads.encode_diagonals gives the batched encoding of the matrix's diagonals over [0, l) u P."""
import numpy as np
import pytest

from util import primes_of

pytestmark = pytest.mark.gpu

NAME = "hyb12_a2"
BITS = [60, 40, 40, 40, 40, 40, 60, 60]
SCALE = 2.0 ** 40


def _both(gpu):
    import phantom_fhe_amd as P
    from phantom_fhe_amd import pyPhantom as ph
    log_n, primes, size_p = primes_of(NAME)
    n = 1 << log_n
    parms = ph.params(ph.scheme_type.ckks)
    parms.set_poly_modulus_degree(n)
    parms.set_special_modulus_size(size_p)
    parms.set_coeff_modulus(ph.create_coeff_modulus(n, BITS))
    hctx = ph.context(parms)
    ctx = P.PhantomContext(log_n, list(primes), size_p, device=gpu)
    return P, ph, hctx, ph.ckks_encoder(hctx), ctx, ctx.ckks_encoder()


def test_mirror_and_pyphantom_equal_the_c_entries(gpu):
    import torch
    P, ph, hctx, henc, ctx, enc = _both(gpu)
    slots = ctx.n // 2
    assert henc.slot_count() == slots == enc.slot_count
    rng = np.random.default_rng(0x1A7E)
    z = rng.uniform(-1, 1, slots) + 1j * rng.uniform(-1, 1, slots)
    for chain_index, size in ((1, slots), (3, slots // 2 + 1), (0, 7)):
        size_Ql = ctx.size_Q if chain_index <= 1 else ctx.size_Q - (chain_index - 1)
        special = chain_index == 0
        pt = henc.encode_complex_vector(hctx, [complex(v) for v in z[:size]], SCALE, chain_index=chain_index)
        assert pt.chain_index() == chain_index and pt.scale() == SCALE
        limbs = size_Ql + (ctx.size_P if special else 0)
        assert pt.coeff_modulus_size() == limbs
        dst = torch.empty((1, limbs, ctx.n), dtype=torch.int64, device=gpu)
        enc.encode_batched(size_Ql, torch.from_numpy(z[None, :size].copy()).to(gpu), size, SCALE, dst, with_special=special)
        assert np.array_equal(pt.to_numpy(), P.to_host(dst)[0]), chain_index
        if special:
            with pytest.raises(ValueError):
                henc.decode_complex_vector(hctx, pt)
            continue
        out = torch.empty((1, slots), dtype=torch.complex128, device=gpu)
        enc.decode_batched(size_Ql, dst, SCALE, out)
        want = out.cpu().numpy()[0]
        got = np.array(henc.decode_complex_vector(hctx, pt))
        assert np.array_equal(got.real.view(np.uint64), want.real.view(np.uint64))
        assert np.array_equal(got.imag.view(np.uint64), want.imag.view(np.uint64))
        assert np.max(np.abs(got[:size] - z[:size])) < 2.0 ** -25 and np.max(np.abs(got[size:]), initial=0.0) < 2.0 ** -25
    # the double overloads: real messages, real parts back
    x = rng.uniform(-1, 1, 10)
    pt = henc.encode_double_vector(hctx, [float(v) for v in x], SCALE)
    assert pt.chain_index() == 1
    same = henc.encode_complex_vector(hctx, [complex(v, 0.0) for v in x], SCALE)
    assert np.array_equal(pt.to_numpy(), same.to_numpy())
    back = np.array(henc.decode_double_vector(hctx, pt))
    assert back.shape == (slots,) and np.array_equal(back, np.array(henc.decode_complex_vector(hctx, pt)).real)


def test_reference_example_calls_resolve_and_checks_raise(gpu):
    """The encode / decode calls of the reference's python/examples/ckks.py, as written there."""
    _, ph, context, encoder, _, _ = _both(gpu)
    slot_count = encoder.slot_count()
    msg = [1.0, 2.0, 3.0, 4.0]
    msg += [0.0] * (slot_count - len(msg))
    scale = SCALE
    pt = encoder.encode_double_vector(context, msg, scale, chain_index=1)
    result = encoder.decode_double_vector(context, pt)
    assert len(result) == slot_count and np.max(np.abs(np.array(result) - np.array(msg))) < 2.0 ** -25
    with pytest.raises(ValueError, match="empty"):
        encoder.encode_double_vector(context, [], scale)
    with pytest.raises(ValueError, match="exceeds max slots"):
        encoder.encode_double_vector(context, [0.0] * (slot_count + 1), scale)
    with pytest.raises(ValueError, match="scale out of bounds"):
        encoder.encode_double_vector(context, msg, -1.0)
    with pytest.raises(ValueError, match="too large"):
        encoder.encode_double_vector(context, [1e30] * slot_count, 2.0 ** 50, chain_index=6)
    bfv = ph.params(ph.scheme_type.bfv)
    bfv.set_poly_modulus_degree(4096)
    bfv.set_special_modulus_size(2)
    bfv.set_coeff_modulus(ph.create_coeff_modulus(4096, BITS))
    bfv.set_plain_modulus(ph.create_plain_modulus(4096, 20))
    with pytest.raises(ValueError, match="unsupported scheme"):
        ph.ckks_encoder(ph.context(bfv))


def test_encode_diagonals(gpu):
    import torch
    from phantom_fhe_amd import workloads as W
    P, _, _, _, ctx, enc = _both(gpu)
    slots = ctx.n // 2
    rng = np.random.default_rng(0xD1A6)
    m = rng.uniform(-1, 1, (8, 8))
    size_Ql = 4
    diags = W.encode_diagonals(enc, size_Ql, m, SCALE, steps=[0, 1, 5])
    assert diags.shape == (3, size_Ql + ctx.size_P, ctx.n)
    vals = torch.from_numpy(W.matrix_diagonals(m, slots, [0, 1, 5])).to(gpu)
    want = torch.empty_like(diags)
    enc.encode_batched(size_Ql, vals, slots, SCALE, want, with_special=True)
    assert torch.equal(diags, want)
    back = torch.empty((3, slots), dtype=torch.complex128, device=gpu)
    enc.decode_batched(size_Ql, diags[:, :size_Ql].contiguous(), SCALE, back)
    assert np.max(np.abs(back.cpu().numpy() - W.matrix_diagonals(m, slots, [0, 1, 5]))) < 2.0 ** -25
