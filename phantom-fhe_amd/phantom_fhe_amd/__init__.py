"""phantom_fhe_amd -- MI355X-native RNS polynomial-arithmetic core for PhantomFHE.

Host-side mirror of the reference's hot-path interface over libphantom_amd.so (HIP, gfx950).
There is no CPU fallback: constructing a PhantomContext without the built library or without a
HIP device raises.
"""
from .core import (BatchEncoder, CKKSEncoder, DBaseConverter, PhantomContext, PhantomRelinKey, coeff_modulus_create, fnwt_1d, inwt_1d, random_bytes,  # noqa: F401
                   scheme_type, has_tuning, set_batch_decode_path, set_batch_encode_path, set_ckks_encode_path, set_strict, set_tuning, stream_copy_rate,
                   stream_rate, to_device, to_host)
from .lib import EXP_LIB_PATH, EXPORTED, LIB_PATH, load  # noqa: F401
