// test_prng_spelling.cpp -- the samplers and the seeded key generation through the host mirror, in the reference's spelling
// (#include "prng.cuh": random_bytes, sample_ternary_poly / sample_error_poly / sample_uniform_poly with the table handle in place of
// the launch configuration, sample_uniform_poly_wrap; PhantomRelinKey::generate_seeded / PhantomGaloisKey::generate_seeded).
// usage: test_prng_spelling <in> <out>.  <in>: 20 seeds of 64 bytes (samplers, secret key, 3 x 2 for the relinearization key,
// 2 x 3 x 2 for two Galois keys), then new keys [3][6][N] words.  <out>: the words, in the order written below.  The set is hyb12_a2
// (N = 4096, 6 data + 2 special primes, dnum 3).  Needs a GPU; built and run by tests/test_gpu_prng_host_api.py, which compares the
// words with the restatement and with the C ABI.
#include "context.cuh"
#include "secretkey.h"
#include "ntt.cuh"
#include "prng.cuh"
#include "host/modulus.h"

#include <cstdio>
#include <string>
#include <vector>

using namespace phantom;
using namespace phantom::arith;
using namespace phantom::util;

#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static bool dump(std::FILE *f, const uint64_t *d, size_t count, const cudaStream_t &s) {
    std::vector<uint64_t> h(count);
    if (hipMemcpyAsync(h.data(), d, count * 8, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return false;
    return std::fwrite(h.data(), 8, count, f) == count;
}

int main(int argc, char **argv) {
    REQUIRE(argc == 3);
    const size_t n = 4096, size_QP = 8, size_P = 2, size_Q = 6, dnum = 3, n_seeds = 20, qp_n = size_QP * n;
    std::vector<uint8_t> seeds(n_seeds * 64);
    std::vector<uint64_t> new_keys(3 * size_Q * n);
    std::FILE *in = std::fopen(argv[1], "rb");
    REQUIRE(in != nullptr);
    REQUIRE(std::fread(seeds.data(), 1, seeds.size(), in) == seeds.size());
    REQUIRE(std::fread(new_keys.data(), 8, new_keys.size(), in) == new_keys.size());
    std::fclose(in);

    // random_bytes, both overloads: count bytes, two calls differ
    auto r1 = random_bytes(64), r2 = random_bytes(64);
    REQUIRE(r1.size() == 64 && r2.size() == 64 && r1 != r2);

    EncryptionParameters parms(scheme_type::ckks);
    parms.set_poly_modulus_degree(n);
    parms.set_special_modulus_size(size_P);
    parms.set_coeff_modulus(CoeffModulus::Create(n, {60, 40, 40, 40, 40, 40, 60, 60}));
    PhantomContext context(parms);
    const auto &s = cudaStreamPerThread;
    const DNTTTable &tables = context.gpu_rns_tables();

    auto d_seeds = make_cuda_auto_ptr<uint8_t>(seeds.size(), s);
    auto d_new = make_cuda_auto_ptr<uint64_t>(new_keys.size(), s);
    REQUIRE(hipMemcpyAsync(d_seeds.get(), seeds.data(), seeds.size(), hipMemcpyHostToDevice, s) == hipSuccess);
    REQUIRE(hipMemcpyAsync(d_new.get(), new_keys.data(), new_keys.size() * 8, hipMemcpyHostToDevice, s) == hipSuccess);
    auto d_rand = make_cuda_auto_ptr<uint8_t>(64, s);
    random_bytes(d_rand.get(), 64, s);
    std::vector<uint8_t> back(64);
    REQUIRE(hipMemcpyAsync(back.data(), d_rand.get(), 64, hipMemcpyDeviceToHost, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess);
    REQUIRE(back != r1 && back != std::vector<uint8_t>(64, 0));

    std::FILE *out = std::fopen(argv[2], "wb");
    REQUIRE(out != nullptr);
    const uint8_t *seed0 = d_seeds.get(), *seed_sk = d_seeds.get() + 64, *seeds_relin = d_seeds.get() + 2 * 64,
                  *seeds_galois = d_seeds.get() + (2 + 2 * dnum) * 64;

    // 1. the three samplers over all QP limbs, as gen_secretkey / encrypt_zero_symmetric spell them (src/secretkey.cu:39, :259, :264)
    auto poly = make_cuda_auto_ptr<uint64_t>(qp_n, s);
    sample_ternary_poly(tables, poly.get(), seed0, size_QP, 0, s);
    REQUIRE(dump(out, poly.get(), qp_n, s));
    sample_error_poly(tables, poly.get(), seed0, size_QP, 0, s);
    REQUIRE(dump(out, poly.get(), qp_n, s));
    sample_uniform_poly_wrap(tables, poly.get(), seed0, n, size_QP, s);
    REQUIRE(dump(out, poly.get(), qp_n, s));
    // 2. a start index: limbs [2, 8)
    sample_uniform_poly(tables, poly.get(), seed0, size_QP - 2, 2, s);
    REQUIRE(dump(out, poly.get(), (size_QP - 2) * n, s));
    bool threw = false;
    try { sample_uniform_poly_wrap(tables, poly.get(), seed0, n / 2, size_QP, s); } catch (const std::invalid_argument &) { threw = true; }
    REQUIRE(threw);
    threw = false;
    try { sample_error_poly(tables, poly.get(), seed0, size_QP, 1, s); } catch (const std::invalid_argument &) { threw = true; }   // rows outside the context
    REQUIRE(threw);

    // 3. gen_secretkey (src/secretkey.cu:366-376): the ternary sample, then the forward transform
    auto sk = make_cuda_auto_ptr<uint64_t>(qp_n, s);
    sample_ternary_poly(tables, sk.get(), seed_sk, size_QP, 0, s);
    nwt_2d_radix8_forward_inplace(sk.get(), tables, size_QP, 0, s);
    REQUIRE(dump(out, sk.get(), qp_n, s));

    // 4. gen_relinkey and create_galois_keys from seeds
    PhantomRelinKey relin;
    relin.generate_seeded(context, sk.get(), d_new.get(), seeds_relin, s);
    REQUIRE(relin.generated() && relin.dnum() == dnum);
    for (size_t d = 0; d < dnum; d++) REQUIRE(dump(out, relin.public_key(d).data(), 2 * qp_n, s));
    PhantomGaloisKey galois;
    galois.generate_seeded(context, sk.get(), d_new.get() + size_Q * n, {5, 25}, seeds_galois, s);
    REQUIRE(galois.galois_elts().size() == 2 && galois.galois_elts()[1] == 25);
    for (size_t i = 0; i < 2; i++)
        for (size_t d = 0; d < dnum; d++) REQUIRE(dump(out, galois.get_relin_keys(i).public_key(d).data(), 2 * qp_n, s));
    std::fclose(out);
    std::printf("OK\n");
    return 0;
}
