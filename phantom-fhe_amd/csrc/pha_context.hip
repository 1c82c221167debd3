// pha_context.hip -- host precompute + device tables behind pha_context_t.
//
// Replaces, for the hot path only: PhantomContext's table upload (src/context.cu:170-183,
// include/ntt.cuh:34-129), the SEAL-derived host tables (src/host/ntt.cu:11-56, src/host/rns.cu:282-337,
// 438-497) and the hybrid key-switch part of the DRNSTool constructor (src/rns.cu:66-200).
// Written independently of oracle/ (different inverse / primality / root-search code paths) so the
// two can check each other.  Each prime's tables are computed once and shared by every level
// (the reference recomputes them per ContextData).
// The constants of the per-level tools (Tool, Behz, Hps, HpsQ) and of every converter are computed by the host-only
// functions of pha_rns_tables.h; this file chooses the bases, calls them and uploads.  Nothing is read back from
// the device (pha_context_download_twiddle and the experiments library's placement census excepted).
#include <algorithm>
#include <atomic>
#include <cstring>
#include <thread>

#include "../../include/phantom_amd.h"
#include "pha_internal.h"

namespace pha {

// ------------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------------
static thread_local std::string g_last_error;
void set_last_error(const char *what) { g_last_error = what ? what : ""; }
int translate_exception() {
    try {
        throw;
    } catch (const std::invalid_argument &e) {
        set_last_error(e.what());
        return PHA_ERR_INVALID_ARGUMENT;
    } catch (const std::logic_error &e) {
        set_last_error(e.what());
        return PHA_ERR_LOGIC;
    } catch (const std::exception &e) {
        set_last_error(e.what());
        return PHA_ERR_RUNTIME;
    } catch (...) {
        set_last_error("unknown error");
        return PHA_ERR_RUNTIME;
    }
}

// ------------------------------------------------------------------------------------------------
// host number theory
// ------------------------------------------------------------------------------------------------
// (h_mulmod / h_invmod / h_shoup: pha_rns_tables.h)
u64 h_powmod(u64 a, u64 e, u64 q) {
    u64 r = 1 % q;
    a %= q;
    for (; e; e >>= 1) {
        if (e & 1) r = h_mulmod(r, a, q);
        a = h_mulmod(a, a, q);
    }
    return r;
}
DModulus h_modulus(u64 q) {
    u128 r = (~(u128)0) / q;  // floor(2^128/q) for q not a power of two
    return DModulus{q, (u64)r, (u64)(r >> 64)};
}
uint32_t h_brev(uint32_t x, int bits) {
    uint32_t r = 0;
    for (int i = 0; i < bits; i++) r |= ((x >> i) & 1u) << (bits - 1 - i);
    return r;
}
bool h_is_prime(u64 n) {
    // deterministic Miller-Rabin, 7-base set valid for all n < 2^64
    if (n < 2) return false;
    static const u64 small[] = {2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37};
    for (u64 p : small) {
        if (n == p) return true;
        if (n % p == 0) return false;
    }
    u64 d = n - 1;
    int s = 0;
    while (!(d & 1)) { d >>= 1; s++; }
    static const u64 bases[] = {2, 325, 9375, 28178, 450775, 9780504, 1795265022};
    for (u64 a : bases) {
        u64 x = h_powmod(a % n, d, n);
        if (x == 0 || x == 1 || x == n - 1) continue;
        bool comp = true;
        for (int i = 1; i < s; i++) {
            x = h_mulmod(x, x, n);
            if (x == n - 1) { comp = false; break; }
        }
        if (comp) return false;
    }
    return true;
}
// minimal primitive degree-th root (degree = 2N a power of two): src/host/numth.cu:309-331.
u64 h_minimal_primitive_root(u64 degree, u64 q) {
    if ((q - 1) % degree) throw std::invalid_argument("invalid modulus in try_minimal_primitive_root");
    const u64 quo = (q - 1) / degree;
    u64 root = 0;
    for (u64 g = 3; g < 4096 && !root; g += 2) {  // any generator-ish start; the minimum is start-independent
        u64 r = h_powmod(g, quo, q);
        if (h_powmod(r, degree >> 1, q) == q - 1) root = r;
    }
    if (!root) throw std::invalid_argument("invalid modulus in try_minimal_primitive_root");
    const u64 sq = h_mulmod(root, root, q);
    u64 cur = root, best = root;
    for (u64 i = 0; i < degree / 2; i++) {  // the degree/2 odd powers are all the primitive roots
        if (cur < best) best = cur;
        cur = h_mulmod(cur, sq, q);
    }
    return best;
}

static void get_primes(u64 ntt_size, int bit_size, size_t count, std::vector<u64> &out) {
    // src/host/numth.cu:207-233
    if (bit_size < 2 || bit_size > 61) throw std::invalid_argument("bit_sizes is invalid");
    const u64 factor = 2 * ntt_size;
    u64 value = (u64)1 << bit_size;
    if (value < factor) throw std::logic_error("failed to find enough qualifying primes");
    value = value - factor + 1;
    const u64 lower = (u64)1 << (bit_size - 1);
    while (count > 0 && value > lower) {
        if (h_is_prime(value)) { out.push_back(value); count--; }
        value -= factor;
    }
    if (count > 0) throw std::logic_error("failed to find enough qualifying primes");
}

// ------------------------------------------------------------------------------------------------
// context
// ------------------------------------------------------------------------------------------------
struct FpTables {
    std::vector<u64> tw, itw;
    std::vector<u64x2> ninv, w1ninv;
    std::vector<FpInfo> info;
};
static u64 fp_bits(u64 w) { return as_u64((double)w); }  // W as a double (exact: W < 2^50)

// Tables of prime c.primes[row] written at position `i` of the output vectors (i == row for the QP chain;
// auxiliary primes are built into short vectors and appended to the device arrays).
static void build_prime_tables(Context &c, uint32_t row, uint32_t i, std::vector<u64x2> &tw, std::vector<u64x2> &itw,
                               std::vector<u64x2> &ninv, std::vector<u64x2> &w1ninv, FpTables &fp) {
    const u64 q = c.primes[row];
    const size_t n = c.n;
    const u64 psi = h_minimal_primitive_root(2 * n, q);
    const u64 ipsi = h_invmod(psi, q);
    c.roots[row] = psi;
    u64x2 *t = tw.data() + (size_t)i * n, *it = itw.data() + (size_t)i * n;
    u64 pw = 1, ipw = 1;
    for (size_t e = 0; e < n; e++) {  // slot brev(e) holds psi^e (src/host/ntt.cu:27-33)
        const uint32_t k = h_brev((uint32_t)e, (int)c.log_n);
        t[k] = u64x2{pw, h_shoup(pw, q)};
        it[k] = u64x2{ipw, h_shoup(ipw, q)};
        pw = h_mulmod(pw, psi, q);
        ipw = h_mulmod(ipw, ipsi, q);
    }
    const u64 ni = h_invmod((u64)(n % q), q);
    c.n_inv[row] = ni;
    ninv[i] = u64x2{ni, h_shoup(ni, q)};
    const u64 w1 = h_mulmod(it[1].x, ni, q);  // what the reference stores in itwiddle[1] (ntt.cu:53-55)
    w1ninv[i] = u64x2{w1, h_shoup(w1, q)};
    // FP64 tables (q < 2^50 only; see pha_arith.h)
    const bool ok = (q >> 50) == 0;
    const FpMod fm = make_fpmod(q);  // ok: bit 0 usable, bit 1 light forward butterflies, bit 2 light inverse ones
    fp.info[i] = FpInfo{fm.q, fm.qinv, ok ? (1u | (fm.ct_light ? 2u : 0u) | (fm.gs_light ? 4u : 0u)) : 0u, 0u};
    if (ok) {
        u64 *tf = fp.tw.data() + (size_t)i * n, *itf = fp.itw.data() + (size_t)i * n;
        for (size_t k = 0; k < n; k++) {
            tf[k] = fp_bits(t[k].x);
            itf[k] = fp_bits(it[k].x);
        }
        fp.ninv[i] = u64x2{fp_bits(ni), 0};
        fp.w1ninv[i] = u64x2{fp_bits(w1), 0};
    }
}

#if defined(PHA_EXPERIMENTS)
// (experiments library only: the one-launch NTT needs it; the product library neither launches the census nor allocates counters)
// XCD placement census: the first workgroup of each class b % 8 records its XCC_ID, the others compare
__global__ void xcd_census_kernel(uint32_t *cls, uint32_t *mismatch) {
    if (threadIdx.x == 0) {
        uint32_t id;
#if defined(__gfx942__) || defined(__gfx950__)
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(id));
#else
        id = blockIdx.x;   // no XCC_ID register: report the classes as if round-robin placement held (one die)
#endif
        const uint32_t mine = (id & 7u) + 1;
        const uint32_t seen = atomicCAS(cls + (blockIdx.x & 7u), 0u, mine);
        if (seen != 0 && seen != mine) atomicAdd(mismatch, 1u);
    }
}
static bool xcd_placement_is_round_robin() {
    DevBuf<uint32_t> d(9);
    for (int rep = 0; rep < 3; rep++) {
        PHA_HIP(hipMemset(d.p, 0, 8 * sizeof(uint32_t)));
        if (rep == 0) PHA_HIP(hipMemset(d.p + 8, 0, sizeof(uint32_t)));
        hipLaunchKernelGGL(xcd_census_kernel, dim3(4096 + 8 * rep + 3), dim3(64), 0, 0, d.p, d.p + 8);
        PHA_HIP(hipGetLastError());
        PHA_HIP(hipDeviceSynchronize());
    }
    uint32_t h[9];
    PHA_HIP(hipMemcpy(h, d.p, sizeof(h), hipMemcpyDeviceToHost));
    return h[8] == 0;
}

// Lazily, the first time the one-launch transform is asked for (pha_set_tuning key 0 bit 9 / key 4): three census launches on
// the null stream and the counter pool.  Not to be triggered inside a stream capture.
bool Context::xcd_placement_round_robin() {
    std::lock_guard<std::mutex> lk(mu);
    if (xcd_checked) return xcd_round_robin;
    DeviceGuard on_device(device);
    xcd_round_robin = xcd_placement_is_round_robin();
    if (xcd_round_robin) {
        flag_pool.alloc(Context::kFlagArenas * (2 * Context::kFlagUnits + 16));
        PHA_HIP(hipMemset(flag_pool.p, 0, flag_pool.count * sizeof(uint32_t)));
    }
    xcd_checked = true;
    return xcd_round_robin;
}
#endif  // PHA_EXPERIMENTS

static void context_init(Context &c, uint32_t log_n, const uint64_t *primes, uint32_t size_qp, uint32_t size_p,
                         int device) {
    if (log_n < 12 || log_n > 17) throw std::invalid_argument("poly_modulus_degree is invalid (2^12..2^17 supported)");
    if (size_qp < 1 || size_qp > 64 || size_p >= size_qp) throw std::invalid_argument("RNSBase is invalid");
    c.device = device;
    DeviceGuard on_device(device);   // the caller's current device is restored when the context has been built
    {
        hipDeviceProp_t prop;
        PHA_HIP(hipGetDeviceProperties(&prop, device));
        c.num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    }
    c.log_n = log_n;
    c.n = (size_t)1 << log_n;
    c.size_qp = size_qp;
    c.size_p = size_p;
    c.size_q = size_qp - size_p;
    c.primes.assign(primes, primes + size_qp);
    c.roots.resize(size_qp);
    c.n_inv.resize(size_qp);
    c.mods.resize(size_qp);
    for (uint32_t i = 0; i < size_qp; i++) {
        const u64 q = c.primes[i];
        if (q >> 61) throw std::invalid_argument("modulus exceeds 61 bits");
        if (!h_is_prime(q) || (q - 1) % (2 * c.n)) throw std::invalid_argument("modulus is not an NTT prime");
        for (uint32_t j = 0; j < i; j++)
            if (c.primes[j] == q) throw std::invalid_argument("coeff_modulus is not coprime");
        c.mods[i] = h_modulus(q);
    }
    std::vector<u64x2> tw((size_t)size_qp * c.n), itw((size_t)size_qp * c.n), ninv(size_qp), w1ninv(size_qp);
    FpTables fp;
    fp.tw.assign((size_t)size_qp * c.n, 0);
    fp.itw.assign((size_t)size_qp * c.n, 0);
    fp.ninv.assign(size_qp, u64x2{0, 0});
    fp.w1ninv.assign(size_qp, u64x2{0, 0});
    fp.info.resize(size_qp);
    {
        const unsigned nthreads = std::max(1u, std::min(std::thread::hardware_concurrency(), size_qp));
        std::vector<std::thread> pool;
        std::vector<std::string> errs(nthreads);
        for (unsigned t = 0; t < nthreads; t++)
            pool.emplace_back([&, t] {
                try {
                    for (uint32_t i = t; i < size_qp; i += nthreads) build_prime_tables(c, i, i, tw, itw, ninv, w1ninv, fp);
                } catch (const std::exception &e) { errs[t] = e.what(); }
            });
        for (auto &th : pool) th.join();
        for (auto &e : errs)
            if (!e.empty()) throw std::invalid_argument(e);
    }
    c.d_mod.upload(c.mods);
    c.d_tw.upload(tw);
    c.d_itw.upload(itw);
    c.d_ninv.upload(ninv);
    c.d_w1ninv.upload(w1ninv);
    c.d_twf.upload(fp.tw);
    c.d_itwf.upload(fp.itw);
    c.d_ninvf.upload(fp.ninv);
    c.d_w1ninvf.upload(fp.w1ninv);
    c.d_fpinfo.upload(fp.info);
    c.rows = size_qp;
}

// Append auxiliary moduli to the context's prime / table arrays: `ntt_primes` get full NTT tables, then one more
// modulus without tables (m_tilde = 2^32 of BEHZ).  Returns the row of the first one.  Nothing may be in flight.
uint32_t Context::add_aux_moduli(const std::vector<u64> &ntt_primes, u64 table_less_modulus) {
    PHA_HIP(hipSetDevice(device));
    PHA_HIP(hipDeviceSynchronize());
    const uint32_t first = rows, cnt = (uint32_t)ntt_primes.size();
    for (u64 q : ntt_primes) {
        if (q >> 61) throw std::invalid_argument("modulus exceeds 61 bits");
        if (!h_is_prime(q) || (q - 1) % (2 * n)) throw std::invalid_argument("modulus is not an NTT prime");
        // an auxiliary base is only ever converted from and to the data base Q: it must be coprime to Q and within itself.  The
        // special primes and the other auxiliary bases never meet it, and a prime may repeat one of theirs in a row of its own
        // (the base R of the HPS multiplies is the primes just below the smallest q_i, which is where special primes of the
        // data primes' size lie, as in the reference)
        for (uint32_t i = 0; i < size_q; i++)
            if (primes[i] == q) throw std::invalid_argument("coeff_modulus is not coprime");
        for (uint32_t i = first; i < primes.size(); i++)
            if (primes[i] == q) throw std::invalid_argument("coeff_modulus is not coprime");
        primes.push_back(q);
        mods.push_back(h_modulus(q));
    }
    const uint32_t extra = table_less_modulus ? 1u : 0u;
    if (extra) {
        primes.push_back(table_less_modulus);
        mods.push_back(h_modulus(table_less_modulus));
    }
    roots.resize(primes.size());
    n_inv.resize(primes.size());
    const uint32_t total = cnt + extra;
    std::vector<u64x2> tw((size_t)total * n, u64x2{0, 0}), itw((size_t)total * n, u64x2{0, 0}), ninv(total, u64x2{0, 0}),
        w1ninv(total, u64x2{0, 0});
    FpTables fp;
    fp.tw.assign((size_t)total * n, 0);
    fp.itw.assign((size_t)total * n, 0);
    fp.ninv.assign(total, u64x2{0, 0});
    fp.w1ninv.assign(total, u64x2{0, 0});
    fp.info.assign(total, FpInfo{0.0, 0.0, 0u, 0u});
    for (uint32_t i = 0; i < cnt; i++) build_prime_tables(*this, first + i, i, tw, itw, ninv, w1ninv, fp);
    d_mod.append(std::vector<DModulus>(mods.begin() + first, mods.end()));
    d_tw.append(tw);
    d_itw.append(itw);
    d_ninv.append(ninv);
    d_w1ninv.append(w1ninv);
    d_twf.append(fp.tw);
    d_itwf.append(fp.itw);
    d_ninvf.append(fp.ninv);
    d_w1ninvf.append(fp.w1ninv);
    d_fpinfo.append(fp.info);
    rows += total;
    return first;
}

// ---- tools: every constant comes from pha_rns_tables.h (host arithmetic, checked on the CPU); the functions below choose the
//      bases, call it and upload ----

// finish a converter: constants to the device, host copy of the phase-1 factors, device description
void upload_bconv(BConv &b, const Rows &ip, const Rows &op, const BConvTables &t, const BConvPlace &place) {
    b.isz = (uint32_t)ip.size();
    b.osz = (uint32_t)op.size();
    b.iprime = ip;
    b.oprime = op;
    b.split_kind = t.split_kind;
    b.mont = t.mont;
    b.r90 = t.r90;
    b.row_pad = t.row_pad;
    b.place = place;
    b.h_hat_inv = t.hat_inv;
    b.hat_inv.upload(t.hat_inv);
    b.mat.upload(t.mat);
    b.mat30.upload(t.mat30);
    b.oninv.upload(t.oninv);
    b.d_iprime.upload(ip);
    b.d_oprime.upload(op);
    b.dev.upload({b.describe()});
}
void build_bconv(Context &c, BConv &b, const Rows &ip, const Rows &op, const std::vector<u64> *out_scale, u64 in_scale, const BConvPlace &place) {
    upload_bconv(b, ip, op, bconv_tables(c.primes, ip, op, out_scale, in_scale), place);
}
void build_bconv_var1(Context &c, BConv &b, const Rows &ip, const Rows &op, const BConvPlace &place) {
    upload_bconv(b, ip, op, bconv_tables_var1(c.primes, ip, op), place);
}

// DRNSTool constructor, HPS multiply part (src/rns.cu:687-790; converters src/host/rns.cu:282-337,438-466).
Hps &Context::hps() {
    std::lock_guard<std::mutex> lk(mu);
    if (hps_tool) return *hps_tool;
    if (!plain_t) throw std::invalid_argument("bfv multiply needs a plain modulus (pha_context_set_plain_modulus)");
    auto h = std::make_unique<Hps>();
    const uint32_t sq = size_q, sr = size_q + 1;
    h->size_q = sq;
    h->size_r = sr;
    // get_primes_below(n, min q, |R|) src/host/numth.cu:235-263
    u64 minq = primes[0];
    for (uint32_t i = 1; i < sq; i++) minq = std::min(minq, primes[i]);
    std::vector<u64> r;
    {
        const u64 factor = 2 * (u64)n, lower = (u64)1 << (63 - __builtin_clzll(minq));
        for (u64 v = minq - factor; r.size() < sr && v > lower; v -= factor)
            if (h_is_prime(v)) r.push_back(v);
        if (r.size() < sr) throw std::logic_error("failed to find enough qualifying primes 2");
    }
    h->aux0 = add_aux_moduli(r, 0);
    const Rows iq = row_range(0, sq), ir = row_range(h->aux0, sr);
    build_bconv(*this, h->q_to_r, iq, ir);
    build_bconv(*this, h->r_to_q, ir, iq);
    h->q_inv.upload(inverse_doubles(primes, iq));
    h->r_inv.upload(inverse_doubles(primes, ir));
    h->alpha_q_mod_r.upload(alpha_table(primes, iq, ir));
    h->alpha_r_mod_q.upload(alpha_table(primes, ir, iq));
    std::vector<double> frac;   // t/Q scale-and-round into R (rns.cu:727-790)
    std::vector<u64> tab;
    scale_round_tables(primes, iq, ir, plain_t, frac, tab);
    h->frac.upload(frac);
    h->div_mod_r.upload(tab);
    hps_tool = std::move(h);
    return *hps_tool;
}

// DRNSTool constructor, hps_overq part (src/rns.cu:792-885), and for size_ql < |Q| the hps_overq_leveled part with
// |Q| - size_ql levels dropped (:897-975).
HpsQ &Context::hps_overq(uint32_t size_ql) {
    if (size_ql == 0) size_ql = size_q;
    if (size_ql < 1 || size_ql > size_q) throw std::invalid_argument("RNSBase is invalid");
    {
        std::lock_guard<std::mutex> lk(mu);
        auto it = hpsq_tools.find(size_ql);
        if (it != hpsq_tools.end()) return *it->second;
    }
    Hps &base = hps();                       // its base R starts with the primes of every Rl (same get_primes_below walk)
    std::lock_guard<std::mutex> lk(mu);
    {
        auto it = hpsq_tools.find(size_ql);
        if (it != hpsq_tools.end()) return *it->second;
    }
    auto h = std::make_unique<HpsQ>();
    const uint32_t sq = size_ql, sr = size_ql, drop = size_q - size_ql;
    h->size_q = sq;
    h->size_r = sr;
    h->size_q_full = size_q;
    h->drop = drop;
    h->aux0 = base.aux0;
    const Rows iq = row_range(0, sq), ir = row_range(h->aux0, sr), dropped = row_range(sq, drop);
    build_bconv(*this, h->q_to_r, iq, ir);
    build_bconv(*this, h->r_to_q, ir, iq);
    build_bconv_var1(*this, h->q_to_r_var1, drop ? row_range(0, size_q) : iq, ir);
    h->q_inv.upload(inverse_doubles(primes, iq));
    h->r_inv.upload(inverse_doubles(primes, ir));
    h->alpha_q_mod_r.upload(alpha_table(primes, iq, ir));
    h->alpha_r_mod_q.upload(alpha_table(primes, ir, iq));
    std::vector<double> frac;
    std::vector<u64> tab;
    scale_round_tables(primes, ir, iq, plain_t, frac, tab);   // t/Rl scale-and-round into Ql (rns.cu:836-885)
    h->frac.upload(frac);
    h->div_mod_q.upload(tab);
    if (drop) {   // Ql/Q scale-and-round (rns.cu:918-972) and the expansion constants (base_Ql_to_QlDrop_conv.PModq)
        scale_round_tables(primes, dropped, iq, 1, frac, tab);
        h->frac_drop.upload(frac);
        h->div_mod_q_drop.upload(tab);
        const std::vector<u64> dm = prod_mod_limbs(primes, dropped, sq, false);
        h->drop_mod_q.upload(dm);
        h->drop_mod_q_shoup.upload(shoup_of(primes, iq, dm));
    }
    HpsQ &ref = *h;
    hpsq_tools[size_ql] = std::move(h);
    return ref;
}

// DRNSTool constructor, BEHZ part (src/rns.cu:392-560).  Needs the plain modulus; top data level only.
Behz &Context::behz() {
    std::lock_guard<std::mutex> lk(mu);
    if (behz_tool) return *behz_tool;
    if (!plain_t) throw std::invalid_argument("bfv multiply needs a plain modulus (pha_context_set_plain_modulus)");
    auto b = std::make_unique<Behz>();
    b->size_q = size_q;
    b->plain_t = plain_t;
    b->size_b = behz_size_b(primes, size_q, plain_t);
    b->size_bsk = b->size_b + 1;
    // get_primes(n, 61, size_b + 1): m_sk first, then B (rns.cu:413-419); descending from 2^61 - 2n + 1 in steps of 2n
    std::vector<u64> found;
    for (u64 v = ((u64)1 << 61) - 2 * n + 1; found.size() < b->size_b + 1 && v > ((u64)1 << 60); v -= 2 * n)
        if (h_is_prime(v)) found.push_back(v);
    if (found.size() < b->size_b + 1) throw std::logic_error("failed to find enough qualifying primes");
    b->m_sk = found[0];
    std::vector<u64> bsk(found.begin() + 1, found.end());
    bsk.push_back(b->m_sk);
    const u64 m_tilde = (u64)1 << 32;
    b->aux0 = add_aux_moduli(bsk, m_tilde);
    const Rows iq = row_range(0, size_q), ib = row_range(b->aux0, b->size_b), obsk = row_range(b->aux0, b->size_bsk);
    // the Q -> Bsk u {m_tilde} converter is only ever fed m_tilde * x (BEHZ_mul_1): its phase-1 factors carry the m_tilde (:450-465), so
    // the conversion kernel scales on load and no scaled copy of the input is written
    build_bconv(*this, b->q_to_bskmt, iq, row_range(b->aux0, b->size_bsk + 1), nullptr, m_tilde);
    build_bconv(*this, b->q_to_bsk, iq, obsk);
    build_bconv(*this, b->b_to_q, ib, iq);
    build_bconv(*this, b->b_to_msk, ib, Rows{b->aux0 + b->size_b});
    b->mt_qhatinv.upload(b->q_to_bskmt.h_hat_inv);
    const BehzTables t = behz_tables(primes, size_q, b->aux0, b->size_b, plain_t);
    b->inv_prod_q_mod_bsk.upload(t.inv_prod_q_mod_bsk);
    b->inv_mt_mod_bsk.upload(t.inv_mt_mod_bsk);
    b->prod_q_mod_bsk.upload(t.prod_q_mod_bsk);
    b->prod_b_mod_q.upload(t.prod_b_mod_q);
    b->t_qb.upload(t.t_qb);
    b->t_qb_shoup.upload(t.t_qb_shoup);
    b->neg_inv_prod_q_mod_mt = t.neg_inv_prod_q_mod_mt;
    b->inv_prod_b_mod_msk = t.inv_prod_b_mod_msk;
    behz_tool = std::move(b);
    return *behz_tool;
}

Tool &Context::tool(uint32_t size_ql) {
    std::lock_guard<std::mutex> lk(mu);
    auto it = tools.find(size_ql);
    if (it != tools.end()) return *it->second;
    if (size_ql < 1 || size_ql > size_q) throw std::invalid_argument("RNSBase is invalid");
    PHA_HIP(hipSetDevice(device));
    auto t = std::make_unique<Tool>();
    t->size_ql = size_ql;
    t->alpha = size_p;
    t->size_qlp = size_ql + size_p;
    const Rows data = row_range(0, size_ql), special = row_range(size_q, size_p);
    t->qlp_prime = data;
    t->qlp_prime.insert(t->qlp_prime.end(), special.begin(), special.end());
    t->d_qlp_prime.upload(t->qlp_prime);
    if (size_ql > 1) {   // rescale: q_last^-1 mod q_i (rns.cu:66-80)
        const std::vector<u64> v = prod_mod_limbs(primes, Rows{size_ql - 1}, size_ql - 1, true);
        t->inv_q_last.upload(v);
        t->inv_q_last_shoup.upload(shoup_of(primes, data, v));
        t->inv_q_last2.upload(pairs_of(primes, data, v));
    }
    if (size_p) {
        // P mod q_i and P^-1 mod q_i (bigP_mod_q, bigPInv_mod_q rns.cu:110-123)
        const std::vector<u64> pm = prod_mod_limbs(primes, special, size_ql, false);
        t->h_pinv.resize(size_ql);
        for (uint32_t i = 0; i < size_ql; i++) t->h_pinv[i] = h_invmod(pm[i], primes[i]);
        t->p_mod_q2.upload(pairs_of(primes, data, pm));
        t->pinv.upload(t->h_pinv);
        t->pinv_shoup.upload(shoup_of(primes, data, t->h_pinv));
        t->pinv2.upload(pairs_of(primes, data, t->h_pinv));
        // digits (rns.cu:152-190); their phase-1 factors, concatenated, are what the mod-up's inverse transform multiplies by
        const std::vector<DigitTables> digits = digit_tables(primes, t->qlp_prime, size_ql, t->alpha);
        t->beta = (uint32_t)digits.size();
        t->digit.resize(t->beta);
        std::vector<u64> phi, phis;
        for (const u64x2 &h : part_hat_inv(digits)) { phi.push_back(h.x); phis.push_back(h.y); }
        std::vector<BConvDev> dd;
        t->modup_mont30 = true;
        for (uint32_t b = 0; b < t->beta; b++) {
            BConv &d = t->digit[b];
            const uint32_t own = t->alpha * b;   // the digit writes around its own limbs, which the same launch copies verbatim
            upload_bconv(d, digits[b].ip, digits[b].op, digits[b].conv, BConvPlace{own, (uint32_t)digits[b].ip.size(), own, 1});
            dd.push_back(d.describe());
            // the carry-free form the conversion launches may use: the digits' common kind (1 = the 30 / 30 split of the headline
            // sets; 2 / 3 = special bases of 17..32 primes or 61-bit primes, BConv::split_kind), 0 if they differ
            if (b == 0) t->modup_split = d.split_kind;
            else if (d.split_kind != t->modup_split) t->modup_split = 0;
            t->modup_max_osz = std::max(t->modup_max_osz, d.osz);
            t->modup_mont30 = t->modup_mont30 && d.mont30();
        }
        t->modup_mont30 = t->modup_mont30 && t->modup_split == 1;
        t->part_hat_inv.upload(phi);
        t->part_hat_inv_shoup.upload(phis);
        t->d_digit_convs.upload(dd);
        // P -> Ql (rns.cu:196-198) from the P limbs of a [Ql || P] buffer, and the same converter delivering P^-1 * (.) mod q_j
        // (key switch + rescale)
        const BConvPlace from_p{0xffffffffu, 0, size_ql, 0};
        build_bconv(*this, t->p_to_ql, special, data, nullptr, 1, from_p);
        build_bconv(*this, t->p_to_ql_pinv, special, data, &t->h_pinv, 1, from_p);
        {   // the P -> Ql converter's phase-1 factors, addressable by the limb index of a [Ql || P] buffer
            std::vector<u64> v(t->size_qlp, 1), vs(t->size_qlp);
            for (uint32_t i = 0; i < t->size_qlp; i++) vs[i] = h_shoup(1, primes[t->qlp_prime[i]]);
            for (uint32_t i = 0; i < size_p; i++) { v[size_ql + i] = t->p_to_ql.h_hat_inv[i].x; vs[size_ql + i] = t->p_to_ql.h_hat_inv[i].y; }
            t->p_hat_inv_by_limb.upload(v);
            t->p_hat_inv_by_limb_shoup.upload(vs);
        }
        t->split_ok = true;
        for (uint32_t i = 0; i < t->size_qlp; i++)
            if (primes[t->qlp_prime[i]] >> 60) t->split_ok = false;
    }
    if (plain_t) {
        const PlainTables pt = plain_tables(primes, size_ql, special, plain_t);
        t->t_mod = h_modulus(plain_t);
        t->inv_q_last_mod_t = pt.inv_q_last_mod_t;
        if (size_ql > 1) t->q_last_mod_q2.upload(pairs_of(primes, data, pt.q_last_mod_q));
        if (size_p) {
            t->pinv_mod_t = pt.pinv_mod_t;
            t->p_hat_mod_t.upload(pt.p_hat_mod_t);
        }
        t->neg_ql_mod_t = pt.neg_ql_mod_t;
        t->t_inv_mod_q.upload(pt.t_inv_mod_q);
        t->t_inv_mod_q_shoup.upload(shoup_of(primes, data, pt.t_inv_mod_q));
        t->plain_upper_half_increment.upload(pt.plain_upper_half_increment);
        t->bgv_ready = true;
    }
    Tool &ref = *t;
    tools[size_ql] = std::move(t);
    return ref;
}

// ---- per-thread arenas of the sentinel streams ---------------------------------------------------------------------------------
// hipStreamPerThread and the null stream name a different real stream in every host thread, so those two handles get one arena
// per calling thread, keyed by a process-wide thread number (never reused: no two live threads share an arena).  A thread that
// exits gives its arenas back: a thread_local reaper walks the live contexts at thread exit (a pool of short-lived threads no
// longer grows one scratch arena -- hundreds of MB at N = 2^16 -- per thread for the life of the context).
namespace {
std::mutex g_live_mu;
std::vector<Context *> g_live_contexts;
std::atomic<size_t> g_thread_counter{0};

struct ThreadReaper {
    size_t id = 0;
    ~ThreadReaper() {
        if (!id) return;
        // the blocks are unhooked under the locks and freed after them: hipFree waits for the device, and no other caller of any
        // context should stall behind that wait (r03 advisor)
        std::vector<std::unique_ptr<Arena>> dead;
        {
            std::lock_guard<std::mutex> lk(g_live_mu);
            for (Context *c : g_live_contexts) c->release_thread_arenas(id, dead);
        }
        int dev = 0;
        const bool have_dev = hipGetDevice(&dev) == hipSuccess;
        dead.clear();   // (~DevBuf: hipFree; device pointers are valid process-wide, the current device does not matter)
        if (have_dev) (void)hipSetDevice(dev);
    }
};
thread_local ThreadReaper t_reaper;

size_t this_thread_number() {
    if (!t_reaper.id) t_reaper.id = ++g_thread_counter;
    return t_reaper.id;
}
}  // namespace

void register_context(Context *c, bool alive) {
    std::lock_guard<std::mutex> lk(g_live_mu);
    if (alive) g_live_contexts.push_back(c);
    else g_live_contexts.erase(std::remove(g_live_contexts.begin(), g_live_contexts.end(), c), g_live_contexts.end());
}

void Context::release_thread_arenas(size_t thread_number, std::vector<std::unique_ptr<Arena>> &dead) {
    std::lock_guard<std::mutex> lk(mu);
    // (the caller frees `dead` outside the locks; DevBuf's hipFree waits for the device, so nothing the exiting thread enqueued can
    //  still be using a block.  A hipGraph that the thread captured on hipStreamPerThread / the null stream has these pointers baked
    //  in and must not be replayed after the thread has exited: capture on an explicit stream instead -- include/phantom_amd.h)
    for (auto *m : {&arenas, &outer_arenas})
        for (auto it = m->begin(); it != m->end();) {
            if (it->first.second == thread_number) {
                dead.push_back(std::move(it->second));
                it = m->erase(it);
            } else {
                ++it;
            }
        }
}

Context::ArenaKey Context::arena_key(void *stream) {
    const bool sentinel = stream == nullptr || as_stream(stream) == hipStreamPerThread;
    return ArenaKey{stream, sentinel ? this_thread_number() : 0};
}

void Lanes::ensure() {
    if (s[0]) return;
    for (int l = 0; l < 2; l++) {
        PHA_HIP(hipStreamCreateWithFlags(&s[l], hipStreamNonBlocking));
        PHA_HIP(hipEventCreateWithFlags(&join[l], hipEventDisableTiming));
    }
    PHA_HIP(hipEventCreateWithFlags(&fork, hipEventDisableTiming));
}
Lanes::~Lanes() {
    for (int l = 0; l < 2; l++) {
        if (join[l]) (void)hipEventDestroy(join[l]);
        if (s[l]) (void)hipStreamDestroy(s[l]);
    }
    if (fork) (void)hipEventDestroy(fork);
}

u64 *Context::scratch(void *stream, size_t words) {
    std::lock_guard<std::mutex> lk(mu);
    auto &a = arenas[arena_key(stream)];
    if (!a) a = std::make_unique<Arena>();
    if (a->buf.count < words) {
        // growing invalidates earlier pointers: make sure nothing in flight still uses the old block
        PHA_HIP(hipStreamSynchronize(as_stream(stream)));
        a->buf.alloc(words);
    }
    return a->buf.p;
}

uint32_t *Context::ntt_flags(void *stream, size_t units) {
    if (units > kFlagUnits || !flag_pool.p) return nullptr;
    std::lock_guard<std::mutex> lk(mu);
    const ArenaKey key = arena_key(stream);
    auto it = flag_arenas.find(key);
    if (it == flag_arenas.end()) {
        if (flag_arenas.size() >= kFlagArenas) return nullptr;
        it = flag_arenas.emplace(key, (uint32_t)flag_arenas.size()).first;
    }
    return flag_pool.p + (size_t)it->second * (2 * kFlagUnits + 16);
}

u64 *Context::scratch_outer(void *stream, size_t words) {
    std::lock_guard<std::mutex> lk(mu);
    auto &a = outer_arenas[arena_key(stream)];
    if (!a) a = std::make_unique<Arena>();
    if (a->buf.count < words) {
        PHA_HIP(hipStreamSynchronize(as_stream(stream)));
        a->buf.alloc(words);
    }
    return a->buf.p;
}

const uint32_t *Context::galois_table(uint32_t elt) {
    // NTT-domain permutation table, include/galois.cuh:98-113
    std::lock_guard<std::mutex> lk(mu);
    auto it = galois_tables.find(elt);
    if (it != galois_tables.end()) return it->second.p;
    check_galois_elt(*this, elt);
    std::vector<uint32_t> tab(n);
    for (uint32_t i = (uint32_t)n; i < 2 * n; i++) {
        const uint32_t rev = h_brev(i, (int)log_n + 1);
        u64 raw = ((u64)elt * rev) >> 1;
        raw &= (u64)(n - 1);
        tab[i - n] = h_brev((uint32_t)raw, (int)log_n);
    }
    DevBuf<uint32_t> d;
    d.upload(tab);
    const uint32_t *p = d.p;
    galois_tables[elt] = std::move(d);
    return p;
}

}  // namespace pha

using namespace pha;

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
extern "C" {

const char *pha_last_error(void) { return g_last_error.c_str(); }

int pha_coeff_modulus_create(uint64_t n, const int *bit_sizes, size_t count, uint64_t *out) {
    PHA_API_BEGIN
    if (n < 2 || n > 131072 || (n & (n - 1))) throw std::invalid_argument("poly_modulus_degree is invalid");
    if (count > 64) throw std::invalid_argument("bit_sizes is invalid");
    // src/host/modulus.cu:98-109: per size, find `need` primes descending, hand out from the back
    std::map<int, std::vector<u64>> table;
    std::map<int, size_t> need;
    for (size_t i = 0; i < count; i++) need[bit_sizes[i]]++;
    for (auto &kv : need) get_primes(n, kv.first, kv.second, table[kv.first]);
    for (size_t i = 0; i < count; i++) {
        auto &v = table[bit_sizes[i]];
        out[i] = v.back();
        v.pop_back();
    }
    PHA_API_END
}

int pha_context_create(pha_context_t *out, uint32_t log_n, const uint64_t *primes_qp, uint32_t size_qp,
                       uint32_t size_p, int device_id) {
    PHA_API_BEGIN
    if (!out || !primes_qp) throw std::invalid_argument("null argument");
    auto h = std::make_unique<pha_context>();
    context_init(h->c, log_n, primes_qp, size_qp, size_p, device_id);
    register_context(&h->c, true);
    *out = h.release();
    PHA_API_END
}

void pha_context_destroy(pha_context_t ctx) {
    if (!ctx) return;
    register_context(&ctx->c, false);
    (void)hipSetDevice(ctx->c.device);
    (void)hipDeviceSynchronize();
    delete ctx;
}

uint32_t pha_context_log_n(pha_context_t ctx) { return ctx->c.log_n; }
uint32_t pha_context_size_qp(pha_context_t ctx) { return ctx->c.size_qp; }
uint32_t pha_context_size_p(pha_context_t ctx) { return ctx->c.size_p; }

int pha_context_set_plain_modulus(pha_context_t ctx, uint64_t plain_modulus) {
    PHA_CTX_BEGIN(ctx)
    if (!ctx) throw std::invalid_argument("null context");
    Context &c = ctx->c;
    if (plain_modulus == 1 || (plain_modulus >> 60)) throw std::invalid_argument("plain_modulus is not valid");
    auto gcd = [](u64 a, u64 b) {
        while (b) { const u64 r = a % b; a = b; b = r; }
        return a;
    };
    for (u64 q : c.primes)  // every q_i and p_j must be invertible modulo t (rns.cu:207,274)
        if (plain_modulus && gcd(q, plain_modulus) != 1) throw std::logic_error("invalid rns bases");
    std::lock_guard<std::mutex> lk(c.mu);
    if (c.plain_t != plain_modulus) {
        PHA_HIP(hipSetDevice(c.device));
        PHA_HIP(hipDeviceSynchronize());  // per-level tools are rebuilt lazily with the new constants
        c.tools.clear();
        c.behz_tool.reset();   // (their auxiliary table rows stay; a later tool appends fresh ones)
        c.hps_tool.reset();
        c.hpsq_tools.clear();
        c.decrypt_tables.clear();
        c.plain_t = plain_modulus;
    }
    PHA_API_END
}

int pha_context_prime_info(pha_context_t ctx, uint32_t i, uint64_t *value, uint64_t ratio[2], uint64_t *root,
                           uint64_t *n_inv) {
    PHA_CTX_BEGIN(ctx)
    Context &c = ctx->c;
    std::lock_guard<std::mutex> lk(c.mu);   // the auxiliary rows (BFV bases) are appended on first use
    if (i >= c.rows) throw std::invalid_argument("prime index out of range");
    if (value) *value = c.primes[i];
    if (ratio) { ratio[0] = c.mods[i].ratio0; ratio[1] = c.mods[i].ratio1; }
    if (root) *root = c.roots[i];
    if (n_inv) *n_inv = c.n_inv[i];
    PHA_API_END
}

int pha_context_download_twiddle(pha_context_t ctx, uint32_t i, int which, uint64_t *host_out) {
    PHA_CTX_BEGIN(ctx)
    Context &c = ctx->c;
    if (i >= c.size_qp || which < 0 || which > 3) throw std::invalid_argument("bad twiddle selector");
    PHA_HIP(hipSetDevice(c.device));
    std::vector<u64x2> row(c.n);
    const u64x2 *src = (which < 2 ? c.d_tw.p : c.d_itw.p) + (size_t)i * c.n;
    PHA_HIP(hipMemcpy(row.data(), src, c.n * sizeof(u64x2), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < c.n; k++) host_out[k] = (which & 1) ? row[k].y : row[k].x;
    if (which >= 2) {  // present the reference's folded slot 1 (src/host/ntt.cu:53-55)
        const u64 q = c.primes[i];
        const u64 w1 = h_mulmod(row[1].x, c.n_inv[i], q);
        host_out[1] = (which == 2) ? w1 : h_shoup(w1, q);
    }
    PHA_API_END
}

int pha_tool_beta(pha_context_t ctx, uint32_t size_ql, uint32_t *beta) {
    PHA_CTX_BEGIN(ctx)
    *beta = ctx->c.tool(size_ql).beta;
    PHA_API_END
}

}  // extern "C"
