// prng.cuh -- stands in for the reference's include/prng.cuh (installed as include/phantom/prng.cuh): random_bytes (both overloads),
// sample_uniform_poly_wrap, and the samplers sample_ternary_poly / sample_error_poly / sample_uniform_poly as host launchers (first
// argument: the table handle instead of <<<grid, block>>> and the device modulus pointer).
// The declarations live in one header, phantom-fhe_amd/host/phantom.h (the MI355X host mirror over the C ABI of
// include/phantom_amd.h); this file only gives it the reference's file name, so that `#include "prng.cuh"` (with
// -I include/phantom) and `#include <phantom/prng.cuh>` (with -I include) resolve as they do against the reference.
#pragma once
#include "../../phantom-fhe_amd/host/phantom.h"
