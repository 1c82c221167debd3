"""Host-side mirror of the reference's hot-path objects over the C ABI.

Names follow the reference (PhantomContext / DNTTTable launchers in include/ntt.cuh:157-226,
DRNSTool methods in include/rns.cuh:156-205, key_switch_inner_prod / keyswitch_inplace in
include/evaluate.cuh:18-32).  torch is used only as the owner of device memory and of the HIP
stream; every call goes straight to libphantom_amd.so with raw device pointers.
Polynomials are torch.int64 CUDA tensors whose bit patterns are the uint64 residues, limb-major
[limb][coeff] (a ciphertext is [poly][limb][coeff], include/ciphertext.h:15-25).
"""
import ctypes as C
from enum import IntEnum

import numpy as np
import torch

from . import lib as _lib


# which operands a summed-product entry takes (PhantomContext._strides): two ciphertexts per term (op1 dense only), or a plaintext
# [L][N] / a raw bfv plaintext [N] and a ciphertext per term, plus acc
_CT_CT, _PLAIN_CT, _RAW_CT = 0, 1, 2


class scheme_type(IntEnum):  # include/host/encryptionparams.h:19-27
    none = 0
    bfv = 1
    ckks = 2
    bgv = 3


def to_device(arr, device="cuda:0"):
    """numpy uint64 array -> int64 device tensor with the same bits."""
    a = np.ascontiguousarray(arr, dtype=np.uint64)
    return torch.from_numpy(a.view(np.int64)).to(device)


def to_host(t):
    """int64 device tensor -> numpy uint64 array with the same bits."""
    return t.detach().cpu().contiguous().numpy().view(np.uint64)


def _ptr(t):
    if t is None:
        return None
    if not (t.is_cuda and t.is_contiguous() and t.dtype == torch.int64):
        raise ValueError("expected a contiguous torch.int64 CUDA tensor")
    return t.data_ptr()


def _i32ptr(t):
    """Device pointer of a contiguous int32 CUDA tensor (bit counts and noise budgets)."""
    if not (t.is_cuda and t.is_contiguous() and t.dtype == torch.int32):
        raise ValueError("expected a contiguous torch.int32 CUDA tensor")
    return t.data_ptr()


def _fptr(t):
    """Device pointer of a contiguous float64 / complex128 CUDA tensor (the CKKS encoder's messages and coefficients)."""
    if not (t.is_cuda and t.is_contiguous() and t.dtype in (torch.float64, torch.complex128)):
        raise ValueError("expected a contiguous torch.float64 or torch.complex128 CUDA tensor")
    return t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _sptr(t, count):
    """Device pointer of `count` 64-byte seeds: a contiguous torch.uint8 CUDA tensor of at least 64 * count bytes."""
    if t is None:
        return None
    if not (t.is_cuda and t.is_contiguous() and t.dtype == torch.uint8):
        raise ValueError("expected a contiguous torch.uint8 CUDA tensor of 64-byte seeds")
    if t.numel() < 64 * int(count):
        raise ValueError(f"{int(count)} seed(s) need {64 * int(count)} bytes, the tensor holds {t.numel()}")
    return t.data_ptr()


def random_bytes(count):
    """random_bytes (src/prng.cu): `count` bytes of std::random_device as a bytes object -- the library's one source of entropy."""
    buf = (C.c_ubyte * max(int(count), 1))()
    _lib.check(_lib.load().pha_random_bytes(buf, int(count)))
    return bytes(buf[:int(count)])


def _elts_keys(elts, keys, optional=True):
    """Galois elements and the key tables of their PhantomRelinKeys as the hoisting entries take them; optional: a key may be None
    (element 1 needs none)."""
    tabs = [None if optional and k is None else k.public_keys_ptr.data_ptr() for k in keys]
    return (C.c_uint32 * len(elts))(*[int(e) for e in elts]), (C.c_void_p * len(keys))(*tabs)


def _weight_ptrs(flat, count=None, shape=None):
    """The device pointers of a flat list of weights (None: no such term); count: how many there must be, of `shape`."""
    if count is not None and len(flat) != count:
        raise ValueError(f"weights must be {shape}")
    return (C.c_void_p * len(flat))(*[_ptr(w) for w in flat])


def stream_copy_rate(dst, src, iters=10):
    """bytes per second (read + write) of the library's own 16-byte-per-lane device-to-device copy (phantom_amd_bench.h)."""
    rate = C.c_double()
    nbytes = min(dst.numel() * dst.element_size(), src.numel() * src.element_size())
    _lib.check(_lib.load().pha_time_stream_copy(_ptr(dst), _ptr(src), nbytes - nbytes % 16, iters, _stream(), C.byref(rate)))
    return rate.value


def stream_rate(dst, src, mode, nontemporal=False, iters=10):
    """bytes per second (read + written) of the library's streaming calibration kernels (phantom_amd_bench.h: pha_time_stream):
    mode 0 copy src -> dst, 1 read-only, 2 write-only, 3 in-place read-modify-write of dst."""
    rate = C.c_double()
    nbytes = min(dst.numel() * dst.element_size(), src.numel() * src.element_size())
    _lib.check(_lib.load().pha_time_stream(_ptr(dst), _ptr(src), nbytes - nbytes % 16, int(mode), int(bool(nontemporal)), iters, _stream(),
                                           C.byref(rate)))
    return rate.value


def has_tuning():
    """True when the loaded library is the test-only experiments build (PHA_LIB_OVERRIDE=.../libphantom_amd_exp.so)."""
    return hasattr(_lib.load(), "pha_set_tuning")


def set_tuning(key, value):
    """A/B knob of the experiments library (csrc/pha_experiments.h); results never change.  The product library's kernel
    selection is fixed: it does not export the symbol."""
    if not has_tuning():
        raise RuntimeError("pha_set_tuning exists only in libphantom_amd_exp.so (set PHA_LIB_OVERRIDE to it): "
                           "the product library has one plan per launch shape")
    _lib.check(_lib.load().pha_set_tuning(int(key), int(value)))


def set_strict(on):
    """Strict mode of the library (pha_set_strict): entry points check caller-supplied operands for words >= their modulus and
    raise ValueError instead of computing.  Returns the previous state.  Process-wide; default from PHA_STRICT=1."""
    return bool(_lib.load().pha_set_strict(1 if on else 0))


def set_ckks_encode_path(mode):
    """Measurement hook (phantom_amd_bench.h: pha_ckks_set_encode_path): which path CKKSEncoder.encode_batched takes for coefficients
    that fit a word -- -1 the library's rule per launch shape (default), 0 the decompose kernel followed by the forward transform, 1
    round-and-reduce as the load prologue of the transform's first pass.  The words are the same either way.  Process-wide."""
    _lib.check(_lib.load().pha_ckks_set_encode_path(int(mode)))


def set_batch_encode_path(mode):
    """Measurement hook (phantom_amd_bench.h: pha_batch_set_encode_path): which form BatchEncoder.encode_batched takes -- -1 the
    library's rule per launch shape (default), 0 the permutation kernel followed by the inverse transform, 1 the gather in the
    inverse transform's first load.  The words are the same either way.  Process-wide."""
    _lib.check(_lib.load().pha_batch_set_encode_path(int(mode)))


def set_batch_decode_path(mode):
    """Measurement hook (phantom_amd_bench.h: pha_batch_set_decode_path): which form BatchEncoder.decode_batched takes -- -1 the
    library's rule per launch shape (default), 0 a plain last store followed by the gather kernel, 1 the scatter in the forward
    transform's last store.  The words are the same either way.  Process-wide."""
    _lib.check(_lib.load().pha_batch_set_decode_path(int(mode)))


def coeff_modulus_create(poly_modulus_degree, bit_sizes):
    """CoeffModulus::Create (src/host/modulus.cu:82-111)."""
    L = _lib.load()
    bits = (C.c_int * len(bit_sizes))(*bit_sizes)
    out = np.zeros(len(bit_sizes), dtype=np.uint64)
    _lib.check(L.pha_coeff_modulus_create(poly_modulus_degree, bits, len(bit_sizes),
                                          out.ctypes.data_as(_lib.u64p)))
    return out


class PhantomContext:
    """Hot-path state of PhantomContext (src/context.cu:121-232): NTT tables for all QP primes on
    one device plus a lazily built DRNSTool per level."""

    def __init__(self, log_n, coeff_modulus, special_modulus_size, device=0):
        self._L = _lib.load()
        self.log_n = int(log_n)
        self.n = 1 << self.log_n
        self.coeff_modulus = np.ascontiguousarray(coeff_modulus, dtype=np.uint64)
        self.size_QP = len(self.coeff_modulus)
        self.size_P = int(special_modulus_size)
        self.size_Q = self.size_QP - self.size_P
        self.device = torch.device("cuda", device) if not isinstance(device, torch.device) else device
        if not torch.cuda.is_available():
            raise RuntimeError("phantom_fhe_amd needs a HIP device; there is no CPU path")
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self._L.pha_context_create(C.byref(h), self.log_n,
                                                  self.coeff_modulus.ctypes.data_as(_lib.u64p),
                                                  self.size_QP, self.size_P, self.device.index or 0))
        self._h = h

    def set_plain_modulus(self, plain_modulus):
        """EncryptionParameters::set_plain_modulus as DRNSTool sees it (src/rns.cu:196-285, BGV constants)."""
        _lib.check(self._L.pha_context_set_plain_modulus(self._h, int(plain_modulus)))
        self.plain_modulus = int(plain_modulus)
        return self

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._L.pha_context_destroy(h)
            self._h = None

    # -- the canonical-operand precondition, checkable (include/phantom_amd.h; csrc/pha_check.hip) --------------------
    def check_canonical(self, data, cms, start=0, size_P_tail=0, polys=1, poly_stride=0):
        """Number of words of data [polys][cms][N] that are >= their limb's modulus (synchronises the stream)."""
        bad = C.c_uint64()
        _lib.check(self._L.pha_check_canonical(self._h, _ptr(data), cms, start, size_P_tail, polys, poly_stride, C.byref(bad), _stream()))
        return bad.value

    def check_canonical_keys(self, size_Ql, keys_ptr, n_keys):
        """The same for the limbs a key switch at level size_Ql reads of n_keys keys (keys_ptr: PhantomRelinKey.public_keys_ptr)."""
        bad = C.c_uint64()
        _lib.check(self._L.pha_check_canonical_keys(self._h, size_Ql, _ptr(keys_ptr), n_keys, C.byref(bad), _stream()))
        return bad.value

    # -- table queries ------------------------------------------------------------------------
    def prime_info(self, idx):
        v, root, ninv = C.c_uint64(), C.c_uint64(), C.c_uint64()
        ratio = (C.c_uint64 * 2)()
        _lib.check(self._L.pha_context_prime_info(self._h, idx, C.byref(v), ratio, C.byref(root), C.byref(ninv)))
        return {"value": v.value, "const_ratio": (ratio[0], ratio[1]), "root": root.value, "n_inv": ninv.value}

    def twiddle_row(self, idx, which):
        out = np.zeros(self.n, dtype=np.uint64)
        _lib.check(self._L.pha_context_download_twiddle(self._h, idx, which, out.ctypes.data_as(_lib.u64p)))
        return out

    def beta(self, size_Ql):
        b = C.c_uint32()
        _lib.check(self._L.pha_tool_beta(self._h, size_Ql, C.byref(b)))
        return b.value

    # -- NTT launchers (include/ntt.cuh:178-226) ------------------------------------------------
    def nwt_2d_radix8_forward_inplace(self, inout, coeff_modulus_size, start_modulus_idx=0):
        _lib.check(self._L.pha_nwt_2d_radix8_forward_inplace(self._h, _ptr(inout), coeff_modulus_size,
                                                             start_modulus_idx, _stream()))

    def nwt_2d_radix8_forward_inplace_include_special_mod(self, inout, cms, start, size_QP, size_P):
        _lib.check(self._L.pha_nwt_2d_radix8_forward_inplace_include_special_mod(
            self._h, _ptr(inout), cms, start, size_QP, size_P, _stream()))

    def nwt_2d_radix8_forward_inplace_include_special_mod_exclude_range(self, inout, cms, start, size_QP,
                                                                       size_P, ex_start, ex_end):
        _lib.check(self._L.pha_nwt_2d_radix8_forward_inplace_include_special_mod_exclude_range(
            self._h, _ptr(inout), cms, start, size_QP, size_P, ex_start, ex_end, _stream()))

    def nwt_2d_radix8_forward_inplace_fuse_moddown(self, ct, cx, bigPInv_mod_q, bigPInv_mod_q_shoup, delta,
                                                   cms, start=0):
        _lib.check(self._L.pha_nwt_2d_radix8_forward_inplace_fuse_moddown(
            self._h, _ptr(ct), _ptr(cx), _ptr(bigPInv_mod_q), _ptr(bigPInv_mod_q_shoup), _ptr(delta), cms,
            start, _stream()))

    def nwt_2d_radix8_backward_inplace(self, inout, coeff_modulus_size, start_modulus_idx=0):
        _lib.check(self._L.pha_nwt_2d_radix8_backward_inplace(self._h, _ptr(inout), coeff_modulus_size,
                                                              start_modulus_idx, _stream()))

    def nwt_2d_radix8_forward_inplace_batched(self, inout, coeff_modulus_size, start_modulus_idx, batch, poly_stride):
        """Extension: the same limbs of `batch` polynomials (poly_stride elements apart) in one launch."""
        _lib.check(self._L.pha_nwt_2d_radix8_forward_inplace_batched(self._h, _ptr(inout), coeff_modulus_size,
                                                                     start_modulus_idx, batch, poly_stride, _stream()))

    def nwt_2d_radix8_backward_inplace_batched(self, inout, coeff_modulus_size, start_modulus_idx, batch, poly_stride):
        _lib.check(self._L.pha_nwt_2d_radix8_backward_inplace_batched(self._h, _ptr(inout), coeff_modulus_size,
                                                                      start_modulus_idx, batch, poly_stride, _stream()))

    def nwt_2d_radix8_backward(self, out, inp, coeff_modulus_size, start_modulus_idx=0):
        _lib.check(self._L.pha_nwt_2d_radix8_backward(self._h, _ptr(out), _ptr(inp), coeff_modulus_size,
                                                      start_modulus_idx, _stream()))

    def nwt_2d_radix8_backward_scale(self, out, inp, cms, start, scale, scale_shoup):
        _lib.check(self._L.pha_nwt_2d_radix8_backward_scale(self._h, _ptr(out), _ptr(inp), cms, start,
                                                            _ptr(scale), _ptr(scale_shoup), _stream()))

    def nwt_2d_radix8_backward_inplace_scale(self, inout, cms, start, scale, scale_shoup):
        """include/ntt.cuh:217 (src/ntt/intt_2d.cu:759-794): inverse NTT in place, every output times the per-limb scale[i]."""
        _lib.check(self._L.pha_nwt_2d_radix8_backward_inplace_scale(self._h, _ptr(inout), cms, start,
                                                                    _ptr(scale), _ptr(scale_shoup), _stream()))

    def nwt_2d_radix8_backward_inplace_include_special_mod(self, inout, cms, start, size_QP, size_P):
        _lib.check(self._L.pha_nwt_2d_radix8_backward_inplace_include_special_mod(
            self._h, _ptr(inout), cms, start, size_QP, size_P, _stream()))

    # -- dyadic kernels (include/polymath.cuh) ------------------------------------------------
    def add_rns_poly(self, a, b, r, cms, mod_start=0):
        _lib.check(self._L.pha_add_rns_poly(self._h, _ptr(a), _ptr(b), _ptr(r), cms, mod_start, _stream()))

    def sub_rns_poly(self, a, b, r, cms, mod_start=0):
        _lib.check(self._L.pha_sub_rns_poly(self._h, _ptr(a), _ptr(b), _ptr(r), cms, mod_start, _stream()))

    def negate_rns_poly(self, a, r, cms, mod_start=0):
        _lib.check(self._L.pha_negate_rns_poly(self._h, _ptr(a), _ptr(r), cms, mod_start, _stream()))

    def multiply_rns_poly(self, a, b, r, cms, mod_start=0):
        _lib.check(self._L.pha_multiply_rns_poly(self._h, _ptr(a), _ptr(b), _ptr(r), cms, mod_start, _stream()))

    def multiply_and_add_rns_poly(self, a, b, d, r, cms, mod_start=0):
        _lib.check(self._L.pha_multiply_and_add_rns_poly(self._h, _ptr(a), _ptr(b), _ptr(d), _ptr(r), cms,
                                                         mod_start, _stream()))

    def multiply_scalar_rns_poly(self, a, scalar, scalar_shoup, r, cms, mod_start=0):
        _lib.check(self._L.pha_multiply_scalar_rns_poly(self._h, _ptr(a), _ptr(scalar), _ptr(scalar_shoup),
                                                        _ptr(r), cms, mod_start, _stream()))

    # -- the rest of polymath.cu (kernels around the hot path: encryption / decryption / plaintext layers) --------
    def add_std_cipher(self, c1, c2, r, cms):
        _lib.check(self._L.pha_add_std_cipher(self._h, _ptr(c1), _ptr(c2), _ptr(r), cms, _stream()))

    def add_and_negate_rns_poly(self, a, b, r, cms, mod_start=0):
        _lib.check(self._L.pha_add_and_negate_rns_poly(self._h, _ptr(a), _ptr(b), _ptr(r), cms, mod_start, _stream()))

    def add_many_rns_poly(self, operands, r, poly_index, cms):
        tab = (C.c_void_p * len(operands))(*[_ptr(o) for o in operands])
        _lib.check(self._L.pha_add_many_rns_poly(self._h, tab, len(operands), _ptr(r), poly_index, cms, _stream()))

    def multiply_uniform_scalar_rns_poly(self, a, scale, r, cms, mod_start=0):
        _lib.check(self._L.pha_multiply_uniform_scalar_rns_poly(self._h, _ptr(a), int(scale), _ptr(r), cms, mod_start, _stream()))

    def multiply_scalar_and_add_rns_poly(self, a, b, scalar, r, cms, mod_start=0):
        _lib.check(self._L.pha_multiply_scalar_and_add_rns_poly(self._h, _ptr(a), _ptr(b), int(scalar), _ptr(r), cms, mod_start, _stream()))

    def multiply_scalar_and_sub_rns_poly(self, a, b, scalar, r, cms, mod_start=0):
        _lib.check(self._L.pha_multiply_scalar_and_sub_rns_poly(self._h, _ptr(a), _ptr(b), int(scalar), _ptr(r), cms, mod_start, _stream()))

    def multiply_and_scale_add_rns_poly(self, a, b, d, scale, r, cms, mod_start=0):
        _lib.check(self._L.pha_multiply_and_scale_add_rns_poly(self._h, _ptr(a), _ptr(b), _ptr(d), int(scale), _ptr(r), cms, mod_start, _stream()))

    def multiply_and_add_negate_rns_poly(self, a, b, d, r, cms, mod_start=0):
        _lib.check(self._L.pha_multiply_and_add_negate_rns_poly(self._h, _ptr(a), _ptr(b), _ptr(d), _ptr(r), cms, mod_start, _stream()))

    def sub_and_scale_rns_poly(self, a, b, scale, scale_shoup, r, cms, mod_start=0):
        _lib.check(self._L.pha_sub_and_scale_rns_poly(self._h, _ptr(a), _ptr(b), _ptr(scale), _ptr(scale_shoup), _ptr(r), cms, mod_start, _stream()))

    def sub_and_scale_single_mod_poly(self, a, b, scale, scale_shoup, modulus, r):
        _lib.check(self._L.pha_sub_and_scale_single_mod_poly(self._h, _ptr(a), _ptr(b), int(scale), int(scale_shoup), int(modulus), _ptr(r), _stream()))

    def bfv_add_timesQ_overt(self, ct, pt, neg_ql_mod_t, neg_ql_mod_t_shoup, t_inv, t_inv_shoup, t, size_Ql, sub=False):
        f = self._L.pha_bfv_sub_timesQ_overt if sub else self._L.pha_bfv_add_timesQ_overt
        _lib.check(f(self._h, _ptr(ct), _ptr(pt), int(neg_ql_mod_t), int(neg_ql_mod_t_shoup), _ptr(t_inv), _ptr(t_inv_shoup), int(t), size_Ql, _stream()))

    def abs_plain_rns_poly(self, operand, threshold, increment, r, cms):
        _lib.check(self._L.pha_abs_plain_rns_poly(self._h, _ptr(operand), int(threshold), _ptr(increment), _ptr(r), cms, _stream()))

    def tensor_prod_mxn_rns_poly(self, op1, m, op2, n_polys, r, cms):
        _lib.check(self._L.pha_tensor_prod_mxn_rns_poly(self._h, _ptr(op1), m, _ptr(op2), n_polys, _ptr(r), m + n_polys - 1, cms, _stream()))

    def multiply_and_negated_add_rns_poly(self, alpha_sk, m_sk, prod_b_mod_q, operand3, r, cms):
        _lib.check(self._L.pha_multiply_and_negated_add_rns_poly(self._h, _ptr(alpha_sk), int(m_sk), _ptr(prod_b_mod_q), _ptr(operand3), _ptr(r), cms, _stream()))

    def bfv_add_plain(self, size_Ql, ct, plain, subtract=False):
        """multiply_{add,sub}_plain_with_scaling_variant (src/scalingvariant.cu:10-60) on ct[0]."""
        _lib.check(self._L.pha_bfv_add_plain(self._h, size_Ql, _ptr(ct), _ptr(plain), int(bool(subtract)), _stream()))

    def bfv_multiply_plain(self, size_Ql, ct, cipher_size, plain):
        """multiply_plain_normal (src/evaluate.cu:1256-1300)."""
        _lib.check(self._L.pha_bfv_multiply_plain(self._h, size_Ql, _ptr(ct), cipher_size, _ptr(plain), _stream()))

    def bgv_lift_plain(self, size_Ql, plain, out):
        """NTT of a plaintext modulo every q_i (the modup_fuse loop of src/evaluate.cu:1150-1154)."""
        _lib.check(self._L.pha_bgv_lift_plain(self._h, size_Ql, _ptr(plain), _ptr(out), _stream()))

    def tensor_prod_2x2_rns_poly_at(self, op1, op2, result, cms, mod_start):
        """tensor_prod_2x2_rns_poly over table rows mod_start .. (the reference's `modulus` pointer: base Bsk / base R callers)."""
        _lib.check(self._L.pha_tensor_prod_2x2_rns_poly_at(self._h, _ptr(op1), _ptr(op2), _ptr(result), cms, mod_start, _stream()))

    def tensor_square_2x2_rns_poly_at(self, op, result, cms, mod_start):
        _lib.check(self._L.pha_tensor_square_2x2_rns_poly_at(self._h, _ptr(op), _ptr(result), cms, mod_start, _stream()))

    def tensor_prod_2x2_rns_poly(self, op1, op2, result, cms):
        _lib.check(self._L.pha_tensor_prod_2x2_rns_poly(self._h, _ptr(op1), _ptr(op2), _ptr(result), cms, _stream()))

    def tensor_square_2x2_rns_poly(self, op, result, cms):
        _lib.check(self._L.pha_tensor_square_2x2_rns_poly(self._h, _ptr(op), _ptr(result), cms, _stream()))

    def add_to_ct(self, ct, cx, size_Ql):
        _lib.check(self._L.pha_add_to_ct(self._h, _ptr(ct), _ptr(cx), size_Ql, _stream()))

    # -- DRNSTool at level size_Ql (include/rns.cuh:156-205) --------------------------------------
    def bconv_P_to_Ql(self, size_Ql, dst, src):
        _lib.check(self._L.pha_bconv_P_to_Ql(self._h, size_Ql, _ptr(dst), _ptr(src), _stream()))

    def modup(self, size_Ql, dst, cks, scheme):
        _lib.check(self._L.pha_modup(self._h, size_Ql, _ptr(dst), _ptr(cks), int(scheme), _stream()))

    def key_switch_inner_prod(self, size_Ql, p_cx, p_t_mod_up, rlk_ptrs):
        """rlk_ptrs: int64 CUDA tensor holding beta device pointers (PhantomRelinKey::public_keys_ptr())."""
        _lib.check(self._L.pha_key_switch_inner_prod(self._h, size_Ql, _ptr(p_cx), _ptr(p_t_mod_up),
                                                     _ptr(rlk_ptrs), _stream()))

    def moddown_from_NTT(self, size_Ql, ct_i, cx_i, scheme):
        _lib.check(self._L.pha_moddown_from_NTT(self._h, size_Ql, _ptr(ct_i), _ptr(cx_i), int(scheme), _stream()))

    def keyswitch_inplace(self, size_Ql, ct, c2, rlk_ptrs, scheme):
        _lib.check(self._L.pha_keyswitch_inplace(self._h, size_Ql, _ptr(ct), _ptr(c2), _ptr(rlk_ptrs),
                                                 int(scheme), _stream()))

    def keyswitch_inplace_batched(self, size_Ql, ct, c2, batch, rlk_ptrs, scheme):
        """`batch` ciphertexts through one set of launches: ct [batch][2][Ql][N] += KS(c2 [batch][Ql][N])."""
        _lib.check(self._L.pha_keyswitch_inplace_batched(self._h, size_Ql, _ptr(ct), _ptr(c2), batch, _ptr(rlk_ptrs),
                                                         int(scheme), _stream()))

    def keyswitch_rescale(self, size_Ql, ct, c2, rlk_ptrs, dst):
        """dst [2][Ql-1][N] = rescale(ct + keyswitch(c2)) in one call (ckks): bit-identical to keyswitch_inplace followed by
        divide_and_round_q_last_ntt, one forward NTT fewer; ct and c2 are only read."""
        _lib.check(self._L.pha_keyswitch_rescale(self._h, size_Ql, _ptr(ct), _ptr(c2), _ptr(rlk_ptrs), _ptr(dst), _stream()))

    def keyswitch_rescale_batched(self, size_Ql, ct, c2, batch, rlk_ptrs, dst):
        _lib.check(self._L.pha_keyswitch_rescale_batched(self._h, size_Ql, _ptr(ct), _ptr(c2), batch, _ptr(rlk_ptrs), _ptr(dst),
                                                         _stream()))

    def keyswitch_mod_switch(self, size_Ql, ct, c2, rlk_ptrs, dst):
        """dst [2][Ql-1][N] = mod_switch(ct + keyswitch(c2)) in one call (bgv): bit-identical to keyswitch_inplace followed by
        mod_t_and_divide_q_last_ntt, without the forward / inverse transform pair between them; ct and c2 are only read."""
        _lib.check(self._L.pha_keyswitch_mod_switch(self._h, size_Ql, _ptr(ct), _ptr(c2), _ptr(rlk_ptrs), _ptr(dst), _stream()))

    def keyswitch_mod_switch_batched(self, size_Ql, ct, c2, batch, rlk_ptrs, dst):
        _lib.check(self._L.pha_keyswitch_mod_switch_batched(self._h, size_Ql, _ptr(ct), _ptr(c2), batch, _ptr(rlk_ptrs), _ptr(dst),
                                                            _stream()))

    def tensor_prod_2x2_batched(self, op1, op2, res01, res2, cms, batch):
        _lib.check(self._L.pha_tensor_prod_2x2_batched(self._h, _ptr(op1), _ptr(op2), _ptr(res01), _ptr(res2), cms,
                                                       batch, _stream()))

    def _strides(self, a, b, cms, terms, batch, strides, kind):
        """The strides of a summed-product entry in 64-bit words: (a term, a batch, b term, b batch) and, for the plaintext kinds,
        acc's batch stride.  strides None: each operand is dense ([batch][terms] + its element shape) or, with one dimension fewer
        ([terms] + ...), shared by all groups (batch stride 0; not op1 of _CT_CT).  Explicit strides pass through: the operands
        may then be views into larger buffers."""
        if strides is not None:
            if kind == _CT_CT:
                t1, b1, t2, b2 = (int(v) for v in strides)
                return t1, b1, t2, b2
            tp, bp, tc, bc, ba = (int(v) for v in strides)
            return tp, bp, tc, bc, ba
        n = self.n
        cw = 2 * cms * n
        aw = cw if kind == _CT_CT else n if kind == _RAW_CT else cms * n
        ab, bb = terms * aw, terms * cw
        if a is not None and b is not None:     # (the library refuses the null pointer)
            dense_b = (batch, terms, 2, cms, n)
            dense_a = dense_b if kind == _CT_CT else (batch, terms, n) if kind == _RAW_CT else (batch, terms, cms, n)
            shape = tuple(a.shape)
            if shape != dense_a:
                if kind == _CT_CT:
                    raise ValueError("op1 must be [batch][terms][2][L][N] (or pass strides)")
                if shape != dense_a[1:]:
                    dims = "[N]" if kind == _RAW_CT else "[L][N]"
                    raise ValueError("plain must be [batch][terms]%s or, shared by all groups, [terms]%s (or pass strides)" % (dims, dims))
                ab = 0
            shape = tuple(b.shape)
            if shape != dense_b:
                if shape != dense_b[1:]:
                    raise ValueError("%s must be [batch][terms][2][L][N] or, shared by all groups, [terms][2][L][N] (or pass strides)" %
                                     ("op2" if kind == _CT_CT else "ct"))
                bb = 0
        return (aw, ab, cw, bb) if kind == _CT_CT else (aw, ab, cw, bb, cw)

    def tensor_prod_2x2_sum_batched(self, op1, op2, res01, res2, cms, terms, batch, strides=None):
        """Extension: for every group g < batch, (res01[g], res2[g]) = sum over k < terms of tensor_prod_2x2(op1[g][k], op2[g][k]) in
        one launch, every word the canonical residue of the sum; res01 [batch][2][L][N], res2 [batch][L][N].  strides: see
        _strides (with explicit strides op1 / op2 may be views into larger buffers)."""
        t1, b1, t2, b2 = self._strides(op1, op2, cms, terms, batch, strides, _CT_CT)
        _lib.check(self._L.pha_tensor_prod_2x2_sum_batched(self._h, _ptr(op1), _ptr(op2), _ptr(res01), _ptr(res2), cms, terms, batch,
                                                           t1, b1, t2, b2, _stream()))

    def inner_product_relin_rescale_batched(self, size_Ql, op1, op2, terms, batch, rlk_ptrs, dst, strides=None, chunk=0):
        """Extension (ckks): dst [batch][2][Ql-1][N] = rescale(relinearize(sum over k of op1[g][k] * op2[g][k])) with ONE key switch per
        sum; bit-identical to tensor_prod_2x2_sum_batched followed by keyswitch_rescale_batched.  `chunk` groups per set of launches
        (0: the library's default)."""
        t1, b1, t2, b2 = self._strides(op1, op2, size_Ql, terms, batch, strides, _CT_CT)
        _lib.check(self._L.pha_inner_product_relin_rescale_batched(self._h, size_Ql, _ptr(op1), _ptr(op2), terms, batch, t1, b1, t2, b2,
                                                                   _ptr(rlk_ptrs), _ptr(dst), chunk, _stream()))

    def inner_product_relin_batched(self, size_Ql, op1, op2, terms, batch, rlk_ptrs, scheme, dst, strides=None, chunk=0):
        """Extension (ckks / bgv), no rescale: dst [batch][2][Ql][N] = relinearize(sum over k of op1[g][k] * op2[g][k])."""
        t1, b1, t2, b2 = self._strides(op1, op2, size_Ql, terms, batch, strides, _CT_CT)
        _lib.check(self._L.pha_inner_product_relin_batched(self._h, size_Ql, _ptr(op1), _ptr(op2), terms, batch, t1, b1, t2, b2,
                                                           _ptr(rlk_ptrs), int(scheme), _ptr(dst), chunk, _stream()))

    def inner_product_relin_mod_switch_batched(self, size_Ql, op1, op2, terms, batch, rlk_ptrs, dst, strides=None, chunk=0):
        """Extension (bgv): dst [batch][2][Ql-1][N] = mod_switch(relinearize(sum over k of op1[g][k] * op2[g][k])) with ONE key switch
        per sum; bit-identical to tensor_prod_2x2_sum_batched followed by keyswitch_mod_switch_batched."""
        t1, b1, t2, b2 = self._strides(op1, op2, size_Ql, terms, batch, strides, _CT_CT)
        _lib.check(self._L.pha_inner_product_relin_mod_switch_batched(self._h, size_Ql, _ptr(op1), _ptr(op2), terms, batch, t1, b1, t2,
                                                                      b2, _ptr(rlk_ptrs), _ptr(dst), chunk, _stream()))

    def multiply_plain_sum_batched(self, plain, ct, acc, res, cms, terms, batch, strides=None):
        """Extension: for every group g < batch, res[g] = acc[g] + sum over k < terms of plain[g][k] (.) ct[g][k] (both polynomials)
        in one launch, every word the canonical residue of the sum; acc may be None, res [batch][2][L][N] may be acc itself.
        strides: see _strides (with explicit strides the operands may be views into larger buffers)."""
        tp, bp, tc, bc, ba = self._strides(plain, ct, cms, terms, batch, strides, _PLAIN_CT)
        _lib.check(self._L.pha_multiply_plain_sum_batched(self._h, _ptr(plain), _ptr(ct), _ptr(acc), _ptr(res), cms, terms, batch,
                                                          tp, bp, tc, bc, ba, _stream()))

    def plain_inner_product_rescale_batched(self, size_Ql, plain, ct, acc, terms, batch, scheme, dst, strides=None, chunk=0):
        """Extension (ckks / bgv): dst [batch][2][Ql-1][N] = the level drop (rescale / mod switch) of the sums above, ONE per sum;
        bit-identical to multiply_plain_sum_batched followed by divide_and_round_q_last_ntt / mod_t_and_divide_q_last_ntt over
        2 * batch polynomials.  `chunk` groups per set of launches (0: the library's default)."""
        tp, bp, tc, bc, ba = self._strides(plain, ct, size_Ql, terms, batch, strides, _PLAIN_CT)
        _lib.check(self._L.pha_plain_inner_product_rescale_batched(self._h, size_Ql, _ptr(plain), _ptr(ct), _ptr(acc), terms, batch,
                                                                   tp, bp, tc, bc, ba, int(scheme), _ptr(dst), chunk, _stream()))

    def bfv_lift_plain_batched(self, size_Ql, plain, count, out, strides=None):
        """Extension (bfv): out (i) [L][N] = NTT form of the centred lift of plain (i) ([N] words below t) for i < count, the lift
        being the load of the forward transform; word for word abs_plain_rns_poly + nwt_2d_radix8_forward_inplace.  strides:
        (plain, out) in 64-bit words; None: dense plain [count][N] and out [count][L][N]."""
        ps, os_ = (int(v) for v in strides) if strides is not None else (self.n, size_Ql * self.n)
        _lib.check(self._L.pha_bfv_lift_plain_batched(self._h, size_Ql, _ptr(plain), count, ps, _ptr(out), os_, _stream()))

    def bfv_multiply_plain_sum_batched(self, size_Ql, plain_ntt, ct, acc, res, terms, batch, strides=None, chunk=0, slab=0):
        """Extension (bfv): for every group g < batch, res[g] = acc[g] + sum over k < terms of plain[g][k] * ct[g][k] in the ring; ct,
        acc (may be None) and res [batch][2][L][N] in coefficient form, plain (g, k) [L][N] as bfv_lift_plain_batched writes it.
        One forward transform per term, one inverse per sum; word for word the loop of bfv_multiply_plain and add_rns_poly.
        strides: see _strides; `chunk` groups per inverse transform and `slab` terms per sum launch (0: the library's
        defaults) size the work buffer and change no bit."""
        tp, bp, tc, bc, ba = self._strides(plain_ntt, ct, size_Ql, terms, batch, strides, _PLAIN_CT)
        _lib.check(self._L.pha_bfv_multiply_plain_sum_batched(self._h, size_Ql, _ptr(plain_ntt), _ptr(ct), _ptr(acc), _ptr(res), terms,
                                                              batch, tp, bp, tc, bc, ba, chunk, slab, _stream()))

    def bfv_plain_inner_product_batched(self, size_Ql, plain, ct, acc, res, terms, batch, strides=None, chunk=0, slab=0):
        """Extension (bfv): bfv_multiply_plain_sum_batched on RAW plaintexts, plain (g, k) = [N] words below t (what a bfv
        PhantomPlaintext holds), lifted and transformed per slab; bit-identical to bfv_lift_plain_batched followed by
        bfv_multiply_plain_sum_batched."""
        tp, bp, tc, bc, ba = self._strides(plain, ct, size_Ql, terms, batch, strides, _RAW_CT)
        _lib.check(self._L.pha_bfv_plain_inner_product_batched(self._h, size_Ql, _ptr(plain), _ptr(ct), _ptr(acc), _ptr(res), terms,
                                                               batch, tp, bp, tc, bc, ba, chunk, slab, _stream()))

    # -- decryption (csrc/pha_decrypt.hip; src/secretkey.cu:533-691) -------------------------------------
    def secret_key_powers(self, sk_ntt, max_power, out=None):
        """compute_secret_key_array: [max_power][size_QP][N] = s, s^2, ... in NTT form from sk_ntt [size_QP][N] (the array
        generate_one_kswitch_key takes).  Returns `out` (allocated when None)."""
        if out is None:
            out = torch.empty((max(int(max_power), 1), self.size_QP, self.n), dtype=torch.int64, device=self.device)
        _lib.check(self._L.pha_secret_key_powers(self._h, _ptr(sk_ntt), max_power, _ptr(out), _stream()))
        return out

    def _decrypt_layout(self, size_Ql, ct, sk_powers, out_words, cipher_size, batch, n_powers, strides):
        """(cipher_size, batch, ct stride, n_powers, dst stride) of a decrypt call: from ct [batch][cipher_size][L][N] and sk_powers
        [n_powers][size_QP][N] unless given; strides: (ct, dst) in 64-bit words, None: dense."""
        batch = int(ct.shape[0]) if batch is None else int(batch)
        cipher_size = int(ct.shape[1]) if cipher_size is None else int(cipher_size)
        n_powers = int(sk_powers.shape[0]) if n_powers is None else int(n_powers)
        cs, ds = (int(v) for v in strides) if strides is not None else (cipher_size * size_Ql * self.n, out_words)
        return cipher_size, batch, cs, n_powers, ds

    def decrypt_phase_batched(self, size_Ql, ct, sk_powers, dst, cipher_size=None, batch=None, n_powers=None, strides=None):
        """Extension (ckks; the first half of bgv): dst (b) [L][N] = c0 + sum_i c_i (.) s^i of ciphertext b of ct [batch][cipher_size][L][N]
        (NTT form) in one launch; sk_powers as secret_key_powers returns it.  dst may be ct itself (result b in c0 (b)'s place, with
        strides (s, s))."""
        k, B, cs, npw, ds = self._decrypt_layout(size_Ql, ct, sk_powers, size_Ql * self.n, cipher_size, batch, n_powers, strides)
        _lib.check(self._L.pha_decrypt_phase_batched(self._h, size_Ql, _ptr(ct), k, B, cs, _ptr(sk_powers), npw, _ptr(dst), ds, _stream()))

    def bgv_decrypt_batched(self, size_Ql, ct, sk_powers, dst, correction_factors=None, cipher_size=None, batch=None, n_powers=None,
                            strides=None, chunk=0):
        """Extension (bgv): dst (b) [N] words below t = the decryption of ciphertext b (NTT form): phase, inverse transform, exact
        conversion to t times the inverse of correction_factors[b] (host integers; None: all 1).  `chunk` ciphertexts per set of
        launches (0: the library's default) changes no bit."""
        k, B, cs, npw, ds = self._decrypt_layout(size_Ql, ct, sk_powers, self.n, cipher_size, batch, n_powers, strides)
        cf = None if correction_factors is None else (C.c_uint64 * max(len(correction_factors), 1))(*[int(f) for f in correction_factors])
        if cf is not None and len(correction_factors) < B:
            raise ValueError("correction_factors holds fewer words than the batch")
        _lib.check(self._L.pha_bgv_decrypt_batched(self._h, size_Ql, _ptr(ct), k, B, cs, _ptr(sk_powers), npw, cf, _ptr(dst), ds, chunk,
                                                   _stream()))

    def bfv_decrypt_batched(self, size_Ql, ct, sk_powers, dst, cipher_size=None, batch=None, n_powers=None, strides=None, chunk=0):
        """Extension (bfv): dst (b) [N] = round(t x / Q_l) mod t of the phase x of ciphertext b (COEFFICIENT form, only read): one
        forward transform of c_1 .. c_{k-1} per chunk, the phase without c0, one inverse transform that adds c0, the scale-and-round."""
        k, B, cs, npw, ds = self._decrypt_layout(size_Ql, ct, sk_powers, self.n, cipher_size, batch, n_powers, strides)
        _lib.check(self._L.pha_bfv_decrypt_batched(self._h, size_Ql, _ptr(ct), k, B, cs, _ptr(sk_powers), npw, _ptr(dst), ds, chunk,
                                                   _stream()))

    def hps_decrypt_scale_and_round(self, size_Ql, dst, src):
        """DRNSTool::hps_decrypt_scale_and_round (src/rns.cu:1519-1689): src [L][N] (coefficient form) -> dst [N] = round(t x / Q_l) mod t."""
        _lib.check(self._L.pha_hps_decrypt_scale_and_round(self._h, size_Ql, _ptr(dst), _ptr(src), _stream()))

    def decrypt_mod_t(self, size_Ql, dst, src):
        """DRNSTool::decrypt_mod_t: src [L][N] (coefficient form) -> dst [N], the exact conversion to the plain modulus."""
        _lib.check(self._L.pha_decrypt_mod_t(self._h, size_Ql, _ptr(dst), _ptr(src), _stream()))

    # -- noise (csrc/pha_noise.hip; src/secretkey.cu:752-840) --------------------------------------------
    def poly_infty_norm_batched(self, size_Ql, src, bits, norm=None, scalar=1, count=None, stride=None):
        """Extension: the exact infinity norm max_j min(v_j, Q_l - v_j) of polynomial c of src [count][L][N] (coefficient form,
        canonical), v_j the CRT composition of scalar * x mod q_i: bits [count] int32 = its significant bit count, norm [count][L]
        (None: not written) its little-endian 64-bit words.  stride: words between polynomials, None: dense."""
        count = int(src.shape[0]) if count is None else int(count)
        stride = size_Ql * self.n if stride is None else int(stride)
        _lib.check(self._L.pha_poly_infty_norm_batched(self._h, size_Ql, _ptr(src), count, stride, int(scalar), _ptr(norm), _i32ptr(bits),
                                                       _stream()))

    def invariant_noise_budget_batched(self, size_Ql, ct, sk_powers, scheme, budget, norm=None, cipher_size=None, batch=None,
                                       n_powers=None, stride=None, chunk=0):
        """Extension (invariant_noise_budget for a batch): budget [batch] int32 = max(0, bitcount(Q_l) - bitcount(norm) - 1) of
        ciphertext b of ct [batch][cipher_size][L][N] (bfv: coefficient form, norm of t * phase; bgv / ckks: NTT form, norm of the
        phase), norm [batch][L] (None: not written) the exact norm's words.  The ciphertexts are only read; nothing synchronises.
        stride: words between ciphertexts, None: dense; `chunk` ciphertexts per set of launches changes no word."""
        k, B, cs, npw, _ = self._decrypt_layout(size_Ql, ct, sk_powers, 0, cipher_size, batch, n_powers,
                                                None if stride is None else (stride, 0))
        _lib.check(self._L.pha_invariant_noise_budget_batched(self._h, size_Ql, _ptr(ct), k, B, cs, _ptr(sk_powers), npw, int(scheme),
                                                              _i32ptr(budget), _ptr(norm), chunk, _stream()))

    # -- encryption (csrc/pha_encrypt.hip; src/secretkey.cu:11-192, 232-295, 382-395, 463-531) ---------------------
    # Samples (the noise e, the ternary u) are [N] SIGNED int64 words, |v| <= 2^16, one polynomial shared by every limb; the uniform a
    # is already in c1's place in ct (canonical words, taken as NTT form).  Randomness is the caller's.
    def encrypt_zero_symmetric_batched(self, size_Ql, sk_ntt, e, ct, scheme, with_special=False, ntt_form=True, count=None, strides=None):
        """encrypt_zero_symmetric for ct [count][2][rows][N] (rows = size_Ql, plus the special rows with_special): c0 (b) =
        -(a (.) s + NTT(k e (b))) from c1 (b) = a in one forward transform per ciphertext; ntt_form=False: the coefficient form
        (-(iNTT(a (.) s) + e), iNTT(a)).  e [count][N]; strides: (e, ct) in 64-bit words, None: dense."""
        rows = size_Ql + (self.size_P if with_special else 0)
        count = int(ct.shape[0]) if count is None else int(count)
        es, cs = (int(v) for v in strides) if strides is not None else (self.n, 2 * rows * self.n)
        _lib.check(self._L.pha_encrypt_zero_symmetric_batched(self._h, size_Ql, int(bool(with_special)), _ptr(sk_ntt), _ptr(e), es, _ptr(ct),
                                                              cs, count, int(scheme), int(bool(ntt_form)), _stream()))

    def public_key_generate(self, sk_ntt, e, pk, scheme):
        """gen_publickey: pk [2][size_QP][N] holds the uniform a in its second half; its first becomes -(a (.) s + NTT(k e)) over all
        QP rows (encrypt_zero_symmetric_batched at the key level, NTT form)."""
        _lib.check(self._L.pha_public_key_generate(self._h, _ptr(sk_ntt), _ptr(e), _ptr(pk), int(scheme), _stream()))

    def encrypt_symmetric_batched(self, size_Ql, sk_ntt, e, plain, ct, scheme, count=None, strides=None):
        """encrypt_symmetric for ct [count][2][L][N] (c1 (b) holds a): ckks: plain [count][L][N] in NTT form (what the encoder writes),
        added in the transform's store; bgv / bfv: plain [count][N] words below t.  strides: (e, plain, ct), a plain stride of 0
        shares one plaintext; None: dense."""
        count = int(ct.shape[0]) if count is None else int(count)
        pw = size_Ql * self.n if int(scheme) == int(scheme_type.ckks) else self.n
        es, ps, cs = (int(v) for v in strides) if strides is not None else (self.n, pw, 2 * size_Ql * self.n)
        _lib.check(self._L.pha_encrypt_symmetric_batched(self._h, size_Ql, _ptr(sk_ntt), _ptr(e), es, _ptr(plain), ps, _ptr(ct), cs, count,
                                                         int(scheme), _stream()))

    def encrypt_asymmetric_batched(self, size_Ql, pk, u, e, plain, ct, scheme, count=None, strides=None, chunk=0):
        """encrypt_asymmetric for ct [count][2][L][N] (only written): pk [2][size_QP][N] as public_key_generate writes it, u [count][N],
        e [count][2][N]; c_j = pk_j (.) NTT(u) + NTT(k e_j) over Q_l u P, the mod-down of every polynomial, the plaintext step of
        encrypt_symmetric_batched.  strides: (u, e, plain, ct); `chunk` ciphertexts per set of launches (0: the library's default)
        changes no bit."""
        count = int(ct.shape[0]) if count is None else int(count)
        pw = size_Ql * self.n if int(scheme) == int(scheme_type.ckks) else self.n
        us, es, ps, cs = (int(v) for v in strides) if strides is not None else (self.n, 2 * self.n, pw, 2 * size_Ql * self.n)
        _lib.check(self._L.pha_encrypt_asymmetric_batched(self._h, size_Ql, _ptr(pk), _ptr(u), us, _ptr(e), es, _ptr(plain), ps, _ptr(ct),
                                                          cs, count, int(scheme), chunk, _stream()))

    # -- seeded samplers and key generation (csrc/pha_prng.hip; src/prng.cu, src/secretkey.cu:297-460) ---------------
    # A seed is 64 bytes; seed arguments are contiguous torch.uint8 CUDA tensors, [64] or [count][64].  The caller supplies every seed.
    def sample_ternary_poly(self, out, seed, coeff_mod_size, mod_start_idx=0):
        """sample_ternary_poly: out [cms][N] canonical residues of the ternary sample of `seed` over rows [mod_start_idx, + cms)."""
        _lib.check(self._L.pha_sample_ternary_poly(self._h, _ptr(out), _sptr(seed, 1), coeff_mod_size, mod_start_idx, _stream()))

    def sample_error_poly(self, out, seed, coeff_mod_size, mod_start_idx=0):
        """sample_error_poly: out [cms][N] canonical residues of the centred binomial noise (|v| <= 21) of `seed`."""
        _lib.check(self._L.pha_sample_error_poly(self._h, _ptr(out), _sptr(seed, 1), coeff_mod_size, mod_start_idx, _stream()))

    def sample_uniform_poly(self, out, seed, coeff_mod_size, mod_start_idx=0):
        """sample_uniform_poly: out [cms][N] uniform residues by rejection, limb y modulo the prime of row mod_start_idx + y."""
        _lib.check(self._L.pha_sample_uniform_poly(self._h, _ptr(out), _sptr(seed, 1), coeff_mod_size, mod_start_idx, _stream()))

    def sample_ternary_signed_batched(self, seeds, out, count=None, out_stride=None):
        """out (b) = [N] signed int64 words of the ternary sample of seeds[b]: the u of encrypt_asymmetric_batched.  out [count][N]
        unless count / out_stride (64-bit words) say otherwise."""
        count = int(out.shape[0]) if count is None else int(count)
        stride = self.n if out_stride is None else int(out_stride)
        _lib.check(self._L.pha_sample_ternary_signed_batched(self._h, _sptr(seeds, count), count, _ptr(out), stride, _stream()))

    def sample_error_signed_batched(self, seeds, out, count=None, out_stride=None):
        """out (b) = [N] signed int64 words of the noise sample of seeds[b]: the e of the encryption entries (the asymmetric entry's
        [count][2][N] is a batch of 2 * count)."""
        count = int(out.shape[0]) if count is None else int(count)
        stride = self.n if out_stride is None else int(out_stride)
        _lib.check(self._L.pha_sample_error_signed_batched(self._h, _sptr(seeds, count), count, _ptr(out), stride, _stream()))

    def sample_uniform_batched(self, size_Ql, seeds, out, with_special=False, count=None, out_stride=None):
        """out (b) = [rows][N] uniform residues of seeds[b] over rows [0, size_Ql) (u P with_special), at out + b * out_stride words.
        `out` may be a view that starts at c1 of a ciphertext buffer (ct[:, 1] of [count][2][rows][N]): its first element and its
        leading stride are used, a is never copied."""
        rows = size_Ql + (self.size_P if with_special else 0)
        count = int(out.shape[0]) if count is None else int(count)
        stride = int(out_stride) if out_stride is not None else (int(out.stride(0)) if out.dim() == 3 else rows * self.n)
        if not (out.is_cuda and out.dtype == torch.int64 and (out.dim() < 3 or out[0].is_contiguous())):
            raise ValueError("expected torch.int64 CUDA polynomials, each contiguous")
        _lib.check(self._L.pha_sample_uniform_batched(self._h, size_Ql, int(bool(with_special)), _sptr(seeds, count), count,
                                                      out.data_ptr(), stride, _stream()))

    def secret_key_generate(self, seed, sk_ntt=None):
        """gen_secretkey: sk_ntt [size_QP][N] = the forward transform of the ternary sample of `seed` over all QP limbs.  Returns it."""
        if sk_ntt is None:
            sk_ntt = torch.empty((self.size_QP, self.n), dtype=torch.int64, device=self.device)
        _lib.check(self._L.pha_secret_key_generate(self._h, _sptr(seed, 1), _ptr(sk_ntt), _stream()))
        return sk_ntt

    def generate_kswitch_keys_seeded(self, sk_ntt, new_keys_ntt, seeds, scheme, evk=None):
        """n_keys key-switching keys at once (gen_relinkey: new_keys_ntt = s^2; create_galois_keys: galois(s) per element) from
        new_keys_ntt [n_keys][size_Q][N] and seeds [n_keys][dnum][2][64] (uniform seed, noise seed): a and e are sampled on the
        device, one batched zero encryption, P * new_key on each digit's limbs.  evk: the storage [n_keys][dnum][2][size_QP][N]
        (allocated when None).  Returns a list of n_keys PhantomRelinKey over that storage."""
        dnum = self.size_Q // self.size_P
        n_keys = int(new_keys_ntt.shape[0])
        if evk is None:
            evk = torch.empty((n_keys, dnum, 2, self.size_QP, self.n), dtype=torch.int64, device=self.device)
        _lib.check(self._L.pha_generate_kswitch_keys_seeded(self._h, _ptr(sk_ntt), _ptr(new_keys_ntt), n_keys, self.size_Q * self.n,
                                                            _sptr(seeds, 2 * n_keys * dnum), _ptr(evk), 2 * self.size_QP * self.n,
                                                            int(scheme), _stream()))
        return [PhantomRelinKey([evk[k, d] for d in range(dnum)]) for k in range(n_keys)]

    def bfv_multiply_behz(self, ct1, ct2, dst):
        """bfv_multiply_behz (src/evaluate.cu:447-548): [2][Q][N] x [2][Q][N] -> [3][Q][N], coefficient form."""
        _lib.check(self._L.pha_bfv_multiply_behz(self._h, _ptr(ct1), _ptr(ct2), _ptr(dst), _stream()))

    def bfv_multiply_hps(self, ct1, ct2, dst):
        """bfv_multiply_hps, mul_tech hps (src/evaluate.cu:674-818): same shapes as bfv_multiply_behz."""
        _lib.check(self._L.pha_bfv_multiply_hps(self._h, _ptr(ct1), _ptr(ct2), _ptr(dst), _stream()))

    def bfv_multiply_hps_overq(self, ct1, ct2, dst):
        """bfv_multiply_hps, mul_tech hps_overq without dropped levels (src/evaluate.cu:674-818); passing the same
        tensor twice takes the reference's squaring shortcut."""
        _lib.check(self._L.pha_bfv_multiply_hps_overq(self._h, _ptr(ct1), _ptr(ct2), _ptr(dst), _stream()))

    def bfv_multiply_hps_overq_leveled(self, size_Ql, ct1, ct2, dst):
        """bfv_multiply_hps under hps_overq_leveled with size_Q - size_Ql levels dropped; buffers over the full base Q."""
        _lib.check(self._L.pha_bfv_multiply_hps_overq_leveled(self._h, size_Ql, _ptr(ct1), _ptr(ct2), _ptr(dst), _stream()))

    def _bfv_batch(self, ct1, ct2, dst):
        """Batch size of ct1, ct2 [B][2][Q][N] -> dst [B][3][Q][N] (None: the library refuses the null pointer)."""
        if ct1 is None or ct2 is None or dst is None:
            return 1
        shape = (2, self.size_Q, self.n)
        if ct1.dim() != 4 or tuple(ct1.shape[1:]) != shape or tuple(ct2.shape) != tuple(ct1.shape):
            raise ValueError("ct1 and ct2 must be [batch][2][Q][N] with the same batch")
        if tuple(dst.shape) != (ct1.shape[0], 3, self.size_Q, self.n):
            raise ValueError("dst must be [batch][3][Q][N]")
        return ct1.shape[0]

    def bfv_multiply_behz_batched(self, ct1, ct2, dst, chunk=0):
        """Extension: bfv_multiply_behz over a batch, ct1, ct2 [B][2][Q][N] -> dst [B][3][Q][N]; ciphertext b has the single
        entry's bits.  `chunk` pairs per set of launches (0: the library's default); the same tensor twice squares."""
        batch = self._bfv_batch(ct1, ct2, dst)
        if batch == 0:      # an empty batch: nothing to do (empty tensors have no device pointer to hand over)
            return
        _lib.check(self._L.pha_bfv_multiply_behz_batched(self._h, _ptr(ct1), _ptr(ct2), _ptr(dst), batch, chunk, _stream()))

    def bfv_multiply_hps_batched(self, ct1, ct2, dst, chunk=0):
        """Extension: bfv_multiply_hps (mul_tech hps) over a batch; shapes and chunk as bfv_multiply_behz_batched."""
        batch = self._bfv_batch(ct1, ct2, dst)
        if batch == 0:      # an empty batch: nothing to do (empty tensors have no device pointer to hand over)
            return
        _lib.check(self._L.pha_bfv_multiply_hps_batched(self._h, _ptr(ct1), _ptr(ct2), _ptr(dst), batch, chunk, _stream()))

    def bfv_multiply_hps_overq_batched(self, size_Ql, ct1, ct2, dst, chunk=0):
        """Extension: hps_overq (size_Ql == |Q|) or hps_overq_leveled (size_Ql < |Q|) over a batch; buffers over the full base Q."""
        batch = self._bfv_batch(ct1, ct2, dst)
        if batch == 0:      # an empty batch: nothing to do (empty tensors have no device pointer to hand over)
            return
        _lib.check(self._L.pha_bfv_multiply_hps_overq_batched(self._h, size_Ql, _ptr(ct1), _ptr(ct2), _ptr(dst), batch, chunk,
                                                              _stream()))

    def bfv_mul_relin_hps_overq_leveled(self, size_Ql, ct1, ct2, rlk_ptrs, dst):
        """bfv_mul_relin_hps with levels dropped (src/evaluate.cu:822-1027); dst [2][Q][N]."""
        _lib.check(self._L.pha_bfv_mul_relin_hps_overq_leveled(self._h, size_Ql, _ptr(ct1), _ptr(ct2), _ptr(rlk_ptrs), _ptr(dst), _stream()))

    # ---- the DRNSTool steps of the BFV multiplies, one polynomial per call (include/rns.cuh:159-200) ----
    def moddown(self, size_Ql, ct_i, cx_i, scheme):
        """DRNSTool::moddown (src/rns_bconv.cu:712-761): BFV input in coefficient form."""
        _lib.check(self._L.pha_moddown(self._h, size_Ql, _ptr(ct_i), _ptr(cx_i), int(scheme), _stream()))

    def tool_aux_sizes(self, size_Ql):
        """(|Bsk|, |R|, |Rl|) of the level's tool; 0 where the base does not exist at that level."""
        a, b, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
        _lib.check(self._L.pha_tool_aux_sizes(self._h, size_Ql, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def fastbconv_m_tilde(self, size_Ql, dst, src):
        _lib.check(self._L.pha_fastbconv_m_tilde(self._h, size_Ql, _ptr(dst), _ptr(src), _stream()))

    def sm_mrq(self, size_Ql, dst, src):
        _lib.check(self._L.pha_sm_mrq(self._h, size_Ql, _ptr(dst), _ptr(src), _stream()))

    def fast_floor(self, size_Ql, input_base_q, input_base_Bsk, out_base_Bsk):
        _lib.check(self._L.pha_fast_floor(self._h, size_Ql, _ptr(input_base_q), _ptr(input_base_Bsk), _ptr(out_base_Bsk), _stream()))

    def fastbconv_sk(self, size_Ql, input_base_Bsk, out_base_q):
        _lib.check(self._L.pha_fastbconv_sk(self._h, size_Ql, _ptr(input_base_Bsk), _ptr(out_base_q), _stream()))

    def scaleAndRound_HPS_QR_R(self, size_Ql, dst, src):
        _lib.check(self._L.pha_scaleAndRound_HPS_QR_R(self._h, size_Ql, _ptr(dst), _ptr(src), _stream()))

    def scaleAndRound_HPS_QlRl_Ql(self, size_Ql, dst, src):
        _lib.check(self._L.pha_scaleAndRound_HPS_QlRl_Ql(self._h, size_Ql, _ptr(dst), _ptr(src), _stream()))

    def ExpandCRTBasis_Ql_Q_add_to_ct(self, size_Ql, dst, src):
        _lib.check(self._L.pha_ExpandCRTBasis_Ql_Q_add_to_ct(self._h, size_Ql, _ptr(dst), _ptr(src), _stream()))

    def scaleAndRound_HPS_Q_Ql(self, size_Ql, dst, src):
        _lib.check(self._L.pha_scaleAndRound_HPS_Q_Ql(self._h, size_Ql, _ptr(dst), _ptr(src), _stream()))

    def ExpandCRTBasis_Ql_Q(self, size_Ql, dst, src):
        _lib.check(self._L.pha_ExpandCRTBasis_Ql_Q(self._h, size_Ql, _ptr(dst), _ptr(src), _stream()))

    def keyswitch_inplace_bfv_leveled(self, size_Ql, ct, c2, rlk_ptrs):
        """keyswitch_inplace for BFV with levels dropped (src/eval_key_switch.cu:142-147, 170-175); ct [2][Q][N], c2 [Q][N]."""
        _lib.check(self._L.pha_keyswitch_inplace_bfv_leveled(self._h, size_Ql, _ptr(ct), _ptr(c2), _ptr(rlk_ptrs), _stream()))

    def batched_modular_gemm(self, C, A, B, m, n, k, batch, mod_start=0, lda=None, ldb=None, ldc=None):
        """C[z] = A[z] @ B[z] mod q_{mod_start + z}, row-major [batch][m][k] x [batch][k][n] (benchmark/matmul_bench.cu).
        lda, ldb, ldc: the leading dimensions in words (None: the rows are dense, k, n and n); matrix z of A starts at
        z * m * lda, of B at z * k * ldb, of C at z * m * ldc."""
        lda, ldb, ldc = (k if lda is None else lda), (n if ldb is None else ldb), (n if ldc is None else ldc)
        _lib.check(self._L.pha_batched_modular_gemm(self._h, _ptr(C), ldc, _ptr(A), lda, _ptr(B), ldb, m, n, k, batch, mod_start,
                                                    _stream()))

    def hoisting(self, size_Ql, ct, galois_elts, galois_keys, scheme):
        """hoisting_inplace (src/evaluate.cu:1670-1866): ct <- sum_e rotate_e(ct); galois_keys[e] is the
        PhantomRelinKey of Galois element galois_elts[e]."""
        elts, tabs = _elts_keys(galois_elts, galois_keys, optional=False)
        _lib.check(self._L.pha_hoisting(self._h, size_Ql, _ptr(ct), elts, len(galois_elts), tabs, int(scheme), _stream()))

    def hoisting_weighted(self, size_Ql, ct, galois_elts, galois_keys, weights, scheme):
        """Build-defined (BASELINE config 5): ct <- sum_e weights[e] (.) rotate_e(ct); weights[e] is a device
        tensor [Ql + size_P][N] (the plaintext over [Q_l || P], NTT form); galois_keys[e] may be None for element 1."""
        elts, tabs = _elts_keys(galois_elts, galois_keys)
        ws = _weight_ptrs(weights)
        _lib.check(self._L.pha_hoisting_weighted(self._h, size_Ql, _ptr(ct), elts, len(galois_elts), tabs, ws, int(scheme),
                                                 _stream()))

    def hoisting_weighted_bsgs(self, size_Ql, ct, baby_elts, baby_keys, giant_elts, giant_keys, weights, scheme):
        """Baby-step / giant-step form (pha_hoisting_weighted_bsgs): ct <- sum_i rot_{giant_elts[i]}(sum_j weights[i][j] (.)
        rot_{baby_elts[j]}(ct)); weights is a list (per giant step) of lists (per baby step) of device tensors [Ql + size_P][N] or
        None; keys may be None for element 1."""
        be, bk = _elts_keys(baby_elts, baby_keys)
        ge, gk = _elts_keys(giant_elts, giant_keys)
        ws = _weight_ptrs([w for row in weights for w in row], len(baby_elts) * len(giant_elts), "[n_giant][n_baby]")
        _lib.check(self._L.pha_hoisting_weighted_bsgs(self._h, size_Ql, _ptr(ct), be, len(baby_elts), bk, ge, len(giant_elts), gk, ws,
                                                      int(scheme), _stream()))

    def hoisting_weighted_bsgs_blocks(self, size_Ql, ct, baby_elts, baby_keys, giant_elts, giant_keys, weights, out, scheme):
        """Several row blocks that share ct and the keys (pha_hoisting_weighted_bsgs_blocks): weights[block][giant][baby] device
        tensors or None, out [blocks][2][Ql][N]; ct is only read."""
        be, bk = _elts_keys(baby_elts, baby_keys)
        ge, gk = _elts_keys(giant_elts, giant_keys)
        ws = _weight_ptrs([w for blk in weights for row in blk for w in row], len(weights) * len(baby_elts) * len(giant_elts),
                          "[n_blocks][n_giant][n_baby]")
        _lib.check(self._L.pha_hoisting_weighted_bsgs_blocks(self._h, size_Ql, _ptr(ct), len(weights), be, len(baby_elts), bk, ge,
                                                             len(giant_elts), gk, ws, _ptr(out), int(scheme), _stream()))

    def hoisting_batched(self, size_Ql, ct, galois_elts, galois_keys, scheme, out=None, chunk=0):
        """pha_hoisting_batched: out[b] = sum_e rotate_e(ct[b]) for a batch ct [B][2][Ql][N] that shares the Galois keys; every
        out[b] is word for word what hoisting() makes of ct[b].  out=None allocates, out=ct works in place; `chunk` ciphertexts go
        through one set of launches (0: the library's default).  Returns out."""
        if out is None:
            out = torch.empty_like(ct)
        if ct.shape[0] == 0:             # (an empty tensor has no device pointer to hand over)
            return out
        elts, tabs = _elts_keys(galois_elts, galois_keys)
        _lib.check(self._L.pha_hoisting_batched(self._h, size_Ql, _ptr(ct), ct.shape[0], elts, len(galois_elts), tabs, int(scheme),
                                                _ptr(out), chunk, _stream()))
        return out

    def hoisting_weighted_batched(self, size_Ql, ct, galois_elts, galois_keys, weights, scheme, out=None, chunk=0):
        """pha_hoisting_weighted_batched: out[b] = sum_e weights[e] (.) rotate_e(ct[b]) for a batch ct [B][2][Ql][N] that shares the
        Galois keys and the weights (as hoisting_weighted takes them); out, chunk and the result as hoisting_batched."""
        if out is None:
            out = torch.empty_like(ct)
        if ct.shape[0] == 0:             # (an empty tensor has no device pointer to hand over)
            return out
        elts, tabs = _elts_keys(galois_elts, galois_keys)
        ws = _weight_ptrs(weights)
        _lib.check(self._L.pha_hoisting_weighted_batched(self._h, size_Ql, _ptr(ct), ct.shape[0], elts, len(galois_elts), tabs, ws,
                                                         int(scheme), _ptr(out), chunk, _stream()))
        return out

    def hoisting_weighted_bsgs_batched(self, size_Ql, ct, baby_elts, baby_keys, giant_elts, giant_keys, weights, scheme, out=None, chunk=0):
        """pha_hoisting_weighted_bsgs_batched: the baby-step / giant-step form for a batch ct [B][2][Ql][N] that shares the keys and
        the weights [n_giant][n_baby] (as hoisting_weighted_bsgs takes them); every out[b] is word for word what
        hoisting_weighted_bsgs() makes of ct[b].  out=None allocates, out=ct works in place; `chunk` ciphertexts go through one set
        of launches (0: the library's default, 4).  Returns out."""
        if out is None:
            out = torch.empty_like(ct)
        if ct.shape[0] == 0:             # (an empty tensor has no device pointer to hand over)
            return out
        be, bk = _elts_keys(baby_elts, baby_keys)
        ge, gk = _elts_keys(giant_elts, giant_keys)
        ws = _weight_ptrs([w for row in weights for w in row], len(baby_elts) * len(giant_elts), "[n_giant][n_baby]")
        _lib.check(self._L.pha_hoisting_weighted_bsgs_batched(self._h, size_Ql, _ptr(ct), ct.shape[0], be, len(baby_elts), bk, ge,
                                                              len(giant_elts), gk, ws, int(scheme), _ptr(out), chunk, _stream()))
        return out

    def divide_and_round_q_last_ntt(self, size_Ql, src, cipher_size, dst):
        _lib.check(self._L.pha_divide_and_round_q_last_ntt(self._h, size_Ql, _ptr(src), cipher_size, _ptr(dst),
                                                           _stream()))

    def generate_one_kswitch_key(self, sk_ntt, new_key_ntt, a, e, scheme):
        """PhantomSecretKey::generate_one_kswitch_key (src/secretkey.cu:297-341), randomness (a, e) supplied by
        the caller; e is in coefficient form and is clobbered.  Returns a PhantomRelinKey."""
        dnum = self.size_Q // self.size_P
        keys = [torch.empty((2, self.size_QP, self.n), dtype=torch.int64, device=self.device) for _ in range(dnum)]
        rlk = PhantomRelinKey(keys)
        _lib.check(self._L.pha_generate_one_kswitch_key(self._h, _ptr(sk_ntt), _ptr(new_key_ntt), _ptr(a), _ptr(e),
                                                        _ptr(rlk.public_keys_ptr), int(scheme), _stream()))
        return rlk

    def mod_t_and_divide_q_last_ntt(self, size_Ql, src, cipher_size, dst):
        """BGV modulus switch (DRNSTool::mod_t_and_divide_q_last_ntt, src/rns.cu:1210-1236)."""
        _lib.check(self._L.pha_mod_t_and_divide_q_last_ntt(self._h, size_Ql, _ptr(src), cipher_size, _ptr(dst),
                                                           _stream()))

    def divide_and_round_q_last(self, size_Ql, src, cipher_size, dst):
        _lib.check(self._L.pha_divide_and_round_q_last(self._h, size_Ql, _ptr(src), cipher_size, _ptr(dst),
                                                       _stream()))

    # -- Galois (src/galois.cu:67-102) --------------------------------------------------------
    def apply_galois_ntt(self, src, dst, galois_elt, cms):
        _lib.check(self._L.pha_apply_galois_ntt(self._h, _ptr(src), _ptr(dst), galois_elt, cms, _stream()))

    def apply_galois(self, src, dst, galois_elt, cms, mod_start=0):
        _lib.check(self._L.pha_apply_galois(self._h, _ptr(src), _ptr(dst), galois_elt, cms, mod_start, _stream()))

    def nwt_2d_radix8_forward_inplace_include_temp_mod(self, inout, cms, start, total_modulus_size):
        _lib.check(self._L.pha_nwt_2d_radix8_forward_inplace_include_temp_mod(self._h, _ptr(inout), cms, start,
                                                                              total_modulus_size, _stream()))

    def nwt_2d_radix8_backward_inplace_include_temp_mod_scale(self, inout, cms, start, total_modulus_size, scale, scale_shoup):
        _lib.check(self._L.pha_nwt_2d_radix8_backward_inplace_include_temp_mod_scale(
            self._h, _ptr(inout), cms, start, total_modulus_size, _ptr(scale), _ptr(scale_shoup), _stream()))

    def nwt_2d_radix8_forward_modup_fuse(self, out, inp, modulus_index, cms, start=0):
        _lib.check(self._L.pha_nwt_2d_radix8_forward_modup_fuse(self._h, _ptr(out), _ptr(inp), modulus_index, cms, start,
                                                                _stream()))

    def apply_galois_batched(self, src, dst, galois_elt, cms, polys, ntt_form):
        _lib.check(self._L.pha_apply_galois_batched(self._h, _ptr(src), _ptr(dst), galois_elt, cms, polys, int(bool(ntt_form)), _stream()))

    def apply_galois_for_keyswitch(self, src, dst_ct, dst_c2, galois_elt, size_Ql, batch, ntt_form):
        """src [batch][2][Ql][N] -> dst_ct = (galois(c0), 0), dst_c2 [batch][Ql][N] = galois(c1): the operands of the key switch
        of a rotation, in one kernel (build-defined; BASELINE config 4)."""
        _lib.check(self._L.pha_apply_galois_for_keyswitch(self._h, _ptr(src), _ptr(dst_ct), _ptr(dst_c2), galois_elt, size_Ql,
                                                          batch, int(bool(ntt_form)), _stream()))

    def relinearize_rotate_batched(self, size_Ql, ct3, batch, rlk_ptrs, glk_ptrs, galois_elt, scheme, out, chunk=0):
        """BASELINE config 4 in one call: out [batch][2][Ql][N] = rotate(relinearize(ct3 [batch][3][Ql][N])); no copies."""
        _lib.check(self._L.pha_relinearize_rotate_batched(self._h, size_Ql, _ptr(ct3), batch, _ptr(rlk_ptrs), _ptr(glk_ptrs),
                                                          galois_elt, int(scheme), _ptr(out), chunk, _stream()))

    def broadcast_keys(self, key_tensors, root, nccl_comm):
        """RCCL-direct broadcast (pha_broadcast_keys) of a list of equally sized key tensors from rank `root` of the raw
        ncclComm_t handle `nccl_comm` (an integer / ctypes pointer), in place."""
        if not key_tensors:
            return
        words = key_tensors[0].numel()
        if any(k.numel() != words for k in key_tensors):
            raise ValueError("keys of one broadcast must have the same size")
        arr = (C.c_void_p * len(key_tensors))(*[_ptr(k) for k in key_tensors])
        _lib.check(self._L.pha_broadcast_keys(self._h, arr, len(key_tensors), words, int(root), C.c_void_p(nccl_comm), _stream()))

    def arena_count(self):
        """Scratch arenas currently held (phantom_amd_bench.h): one per explicit stream / per live host thread."""
        cnt = C.c_size_t()
        _lib.check(self._L.pha_context_arena_count(self._h, C.byref(cnt)))
        return cnt.value

    # -- CKKS encoder pieces that belong to the level (DRNSBase, src/rns_base.cu:49-253) ------------
    def decompose_array(self, size_Ql, dst, src, max_coeff_bit_count):
        """DRNSBase::decompose_array: dst [size_Ql][N] <- the rounded coefficients of src (N / 2 complex numbers: coefficient j is
        Re src[j], coefficient j + N / 2 is Im src[j]) modulo every prime of the level."""
        _lib.check(self._L.pha_decompose_array(self._h, size_Ql, _ptr(dst), _fptr(src), int(max_coeff_bit_count), _stream()))

    def compose_array(self, size_Ql, dst, src, inv_scale):
        """DRNSBase::compose_array: src [size_Ql][N] in coefficient form -> dst N / 2 complex numbers, the centred CRT value of every
        coefficient times inv_scale."""
        _lib.check(self._L.pha_compose_array(self._h, size_Ql, _fptr(dst), _ptr(src), float(inv_scale), _stream()))

    def ckks_encoder(self):
        """A CKKSEncoder over this context."""
        return CKKSEncoder(self)

    # -- measurement ------------------------------------------------------------------------------
    def repeat_forward_ntt_batched(self, inout, cms, start, batch, poly_stride, repeats):
        """`repeats` back-to-back batched forward transforms enqueued from C (bench.py's timed region)."""
        _lib.check(self._L.pha_repeat_forward_ntt_batched(self._h, _ptr(inout), cms, start, batch, poly_stride, repeats, _stream()))

    def time_forward_ntt(self, inout, cms, iters):
        ms = C.c_float()
        _lib.check(self._L.pha_time_forward_ntt(self._h, _ptr(inout), cms, iters, _stream(), C.byref(ms)))
        return ms.value


class CKKSEncoder:
    """PhantomCKKSEncoder's device work (src/ckks.cu) over the C ABI: the tables, the special FFT launchers, and the batched
    encode / decode extensions.  Messages are contiguous torch.complex128 (or float64 pairs) CUDA tensors."""

    def __init__(self, ctx):
        self._ctx, self._L = ctx, _lib.load()    # the context must outlive the encoder: keep it
        h = C.c_void_p()
        _lib.check(self._L.pha_ckks_encoder_create(ctx._h, C.byref(h)))
        self._h = h
        self.slot_count = ctx.n // 2

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.pha_ckks_encoder_destroy(self._h)
            self._h = None

    def tables(self):
        """(roots [2N] complex128, group [N / 4] uint32): the host tables of the constructor."""
        roots = np.zeros(4 * self.slot_count, dtype=np.complex128)
        group = np.zeros(self.slot_count // 2, dtype=np.uint32)
        _lib.check(self._L.pha_ckks_encoder_tables(self._h, roots.ctypes.data_as(C.POINTER(C.c_double)),
                                                   group.ctypes.data_as(C.POINTER(C.c_uint32))))
        return roots, group

    def special_fft_backward(self, inout, log_n, scalar):
        """special_fft_backward (src/fft.cu:385-422): in place on 2^log_n complex numbers, no bit reversal, times `scalar`."""
        _lib.check(self._L.pha_special_fft_backward(self._h, _fptr(inout), log_n, float(scalar), _stream()))

    def special_fft_forward(self, inout, log_n):
        """special_fft_forward (src/fft.cu:348-379)."""
        _lib.check(self._L.pha_special_fft_forward(self._h, _fptr(inout), log_n, _stream()))

    def encode_batched(self, size_Ql, values, values_size, scale, dst, with_special=False, count=None, strides=None):
        """Extension: plaintext k of dst [count][L][N] (L = size_Ql, or size_Ql + size_P with_special: the limbs [0, size_Ql) u P) <-
        the NTT-form encoding of message k = the first values_size numbers of values [count][...] at `scale`.  strides: (values in
        complex numbers, dst in words); None: dense.  Returns max_coeff_bit_count per message; synchronises the stream once."""
        ctx = self._ctx
        limbs = size_Ql + (ctx.size_P if with_special else 0)
        count = int(values.shape[0]) if count is None else int(count)
        vs, ds = (int(v) for v in strides) if strides is not None else (int(values.numel() // max(count, 1)), limbs * ctx.n)
        bits = (C.c_int * max(count, 1))()
        _lib.check(self._L.pha_ckks_encode_batched(self._h, size_Ql, int(bool(with_special)), _fptr(values), int(values_size), count, vs,
                                                   float(scale), _ptr(dst), ds, bits, _stream()))
        return [int(b) for b in bits[:count]]

    def decode_batched(self, size_Ql, plain, scale, values_out, count=None, strides=None):
        """Extension: values_out [count][N / 2] complex <- the decoding of plaintext k of plain [count][size_Ql][N] (NTT form) at
        `scale`.  strides: (plain in words, values_out in complex numbers); None: dense."""
        ctx = self._ctx
        count = int(plain.shape[0]) if count is None else int(count)
        ps, vs = (int(v) for v in strides) if strides is not None else (size_Ql * ctx.n, self.slot_count)
        _lib.check(self._L.pha_ckks_decode_batched(self._h, size_Ql, _ptr(plain), count, ps, float(scale), _fptr(values_out), vs, _stream()))


class BatchEncoder:
    """PhantomBatchEncoder's device work (src/batchencoder.cu) over the C ABI: the index map, the transforms modulo the plain modulus
    (gpu_plain_tables()), and the batched encode / decode extensions.  Messages and plaintexts are contiguous torch.int64 CUDA
    tensors holding uint64 bit patterns; a plaintext is [N] words below t in coefficient form.  The context needs a plain modulus
    that is a prime = 1 (mod 2N), and must keep it: a call after set_plain_modulus changed it raises ValueError."""

    def __init__(self, ctx):
        self._ctx, self._L = ctx, _lib.load()    # the context must outlive the encoder: keep it
        h = C.c_void_p()
        _lib.check(self._L.pha_batch_encoder_create(ctx._h, C.byref(h)))
        self._h = h
        self.slot_count = ctx.n

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.pha_batch_encoder_destroy(self._h)
            self._h = None

    def index_map(self):
        """matrix_reps_index_map (populate_matrix_reps_index_map, src/batchencoder.cu:25-49): numpy uint64 [N]."""
        out = np.zeros(self.slot_count, dtype=np.uint64)
        _lib.check(self._L.pha_batch_encoder_index_map(self._h, out.ctypes.data_as(_lib.u64p)))
        return out

    def _layout(self, t, count, stride):
        count = (int(t.shape[0]) if t.dim() > 1 else 1) if count is None else int(count)
        return count, self.slot_count if stride is None else int(stride)

    def plain_nwt_forward_inplace_batched(self, inout, count=None, stride=None):
        """nwt_2d_radix8_forward_inplace over gpu_plain_tables() for inout [count][N] (words below t), in place; stride in words,
        None: dense."""
        count, stride = self._layout(inout, count, stride)
        _lib.check(self._L.pha_plain_nwt_forward_inplace_batched(self._h, _ptr(inout), count, stride, _stream()))

    def plain_nwt_backward_inplace_batched(self, inout, count=None, stride=None):
        """nwt_2d_radix8_backward_inplace over gpu_plain_tables() (N^-1 included), in place."""
        count, stride = self._layout(inout, count, stride)
        _lib.check(self._L.pha_plain_nwt_backward_inplace_batched(self._h, _ptr(inout), count, stride, _stream()))

    def encode_batched(self, values, values_size, dst, count=None, strides=None):
        """Extension: plaintext k of dst [count][N] <- the encoding of message k = the first values_size words of values [count][...]
        (slots past values_size are zero; a word with bit 63 set, i.e. a negative int64, gets + t).  strides: (values, dst) in words,
        a values stride of 0 shares one message; None: dense.  No synchronisation."""
        count = (int(dst.shape[0]) if dst.dim() > 1 else 1) if count is None else int(count)
        dense = 0 if values is None else int(values.numel() // max(count, 1))
        vs, ds = (int(v) for v in strides) if strides is not None else (dense, self.slot_count)
        _lib.check(self._L.pha_batch_encode_batched(self._h, _ptr(values), int(values_size), count, vs, _ptr(dst), ds, _stream()))

    def decode_batched(self, plain, values_out, count=None, strides=None):
        """Extension: values_out [count][N] <- the decoding of plaintext k of plain [count][N] (only read).  strides: (plain,
        values_out) in words; None: dense."""
        count = (int(plain.shape[0]) if plain.dim() > 1 else 1) if count is None else int(count)
        ps, vs = (int(v) for v in strides) if strides is not None else (self.slot_count, self.slot_count)
        _lib.check(self._L.pha_batch_decode_batched(self._h, _ptr(plain), count, ps, _ptr(values_out), vs, _stream()))


class DBaseConverter:
    """DBaseConverter (include/rns_bconv.cuh:13-87) between two bases given as rows of the context's prime table."""

    def __init__(self, ctx, ibase, obase=None, out_modulus=None):
        """obase: rows of the prime table; or out_modulus: ONE raw output modulus (the plain modulus t of base_q_to_t_conv_,
        src/rns.cu:283-284) -- such a converter serves exact_convert_array only."""
        self._ctx, self._L = ctx, _lib.load()
        self.ibase = [int(i) for i in ibase]
        ib = (C.c_uint32 * len(self.ibase))(*self.ibase)
        h = C.c_void_p()
        if out_modulus is not None:
            self.obase = None
            _lib.check(self._L.pha_base_converter_create_modulus(ctx._h, ib, len(self.ibase), int(out_modulus), C.byref(h)))
        else:
            self.obase = [int(o) for o in obase]
            ob = (C.c_uint32 * len(self.obase))(*self.obase)
            _lib.check(self._L.pha_base_converter_create(ctx._h, ib, len(self.ibase), ob, len(self.obase), C.byref(h)))
        self._h = h

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.pha_base_converter_destroy(self._h)
            self._h = None

    def bConv_BEHZ(self, dst, src):
        _lib.check(self._L.pha_bConv_BEHZ(self._h, _ptr(dst), _ptr(src), _stream()))

    def bConv_HPS(self, dst, src):
        _lib.check(self._L.pha_bConv_HPS(self._h, _ptr(dst), _ptr(src), _stream()))

    def bConv_BEHZ_var1(self, dst, src):
        """DBaseConverter::bConv_BEHZ_var1 (src/rns_bconv.cu:231-246)."""
        _lib.check(self._L.pha_bConv_BEHZ_var1(self._h, _ptr(dst), _ptr(src), _stream()))

    def exact_convert_array(self, dst, src):
        """DBaseConverter::exact_convert_array (src/rns_bconv.cu:374-431): [ibase][N] -> [N] modulo the one output modulus."""
        _lib.check(self._L.pha_exact_convert_array(self._h, _ptr(dst), _ptr(src), _stream()))


class PhantomRelinKey:
    """Device layout of PhantomRelinKey (include/secretkey.h:102-165): dnum public keys, each
    [2][size_QP][N], plus a device array of their pointers."""

    def __init__(self, keys):
        self.public_keys = [k.contiguous() for k in keys]
        self.public_keys_ptr = torch.tensor([k.data_ptr() for k in self.public_keys], dtype=torch.int64,
                                            device=self.public_keys[0].device)

    @classmethod
    def from_numpy(cls, evk, device="cuda:0"):
        return cls([to_device(evk[i], device) for i in range(evk.shape[0])])


def fnwt_1d(inout, twiddles, twiddles_shoup, modulus, dim, cms, start=0, opt=False):
    """fnwt_1d / fnwt_1d_opt (src/ntt/ntt_1d.cu): modulus is a device tensor of (value, const_ratio lo, hi) triples."""
    L = _lib.load()
    f = L.pha_fnwt_1d_opt if opt else L.pha_fnwt_1d
    _lib.check(f(_ptr(inout), _ptr(twiddles), _ptr(twiddles_shoup), _ptr(modulus), dim, cms, start, _stream()))


def inwt_1d(inout, itwiddles, itwiddles_shoup, modulus, scalar, scalar_shoup, dim, cms, start=0, opt=False):
    L = _lib.load()
    f = L.pha_inwt_1d_opt if opt else L.pha_inwt_1d
    _lib.check(f(_ptr(inout), _ptr(itwiddles), _ptr(itwiddles_shoup), _ptr(modulus), _ptr(scalar), _ptr(scalar_shoup), dim,
                 cms, start, _stream()))
