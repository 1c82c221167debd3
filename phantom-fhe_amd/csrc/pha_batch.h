// pha_batch.h -- the arithmetic and index math of the BFV / BGV batch encoder (src/batchencoder.cu:25-49 the index map, :51-60
// encode_gpu's load rule, :91-95 decode_gpu; the transform of gpu_plain_tables(): src/host/ntt.cu:11-56 tables, include/butterfly.cuh
// :10-37 butterflies): one pass of the negacyclic transform modulo ONE prime t over a tile held in LDS, with the encoder's permutation
// in the first load (encode) or the last store (decode).  Host/device like pha_ckks_fft.h and pha_decrypt.h, so that
// tests/emu/emu_batch.cpp compiles the very source the kernels of pha_batch.hip run -- test-only on the host.
//
// The transform is the SEAL-order radix-2 graph: the forward one (Cooley-Tukey) runs the stages whose pairs are N/2, N/4, .. 1 apart,
// the stage with pairs 2^lp apart taking tw[(N >> (lp + 1)) + (point >> (lp + 1))]; the inverse one (Gentleman-Sande) runs them 1, 2,
// .. N/2 apart with the table of inverse powers, and multiplies by N^-1 in its last store.  tw[k] = psi^brev(k) with its Shoup
// quotient, psi the minimal primitive 2N-th root modulo t.  Words are kept lazy between stages (forward: below 4t, inverse: below
// 2t; t < 2^60, so nothing wraps) and only the last store reduces, so the stored words are the canonical residues whatever the
// tiling: any grouping of the stages that executes this graph gives the same words.  There is ONE arithmetic form for every t (the
// integer Harvey butterflies of pha_arith.h): the modulus and N^-1 are kernel arguments, uniform over the launch.
#pragma once
#include "pha_arith.h"

namespace pha {

enum { NWT_IN_PLAIN = 0, NWT_IN_GATHER = 1 };
enum { NWT_OUT_LAZY = 0, NWT_OUT_CANON = 1, NWT_OUT_SCATTER = 2 };

struct NwtPass {
    const u64 *in;
    u64 *out;
    size_t in_stride, out_stride;   // words between consecutive messages (in_stride 0: one message shared)
    const u64x2 *tw;                // [n] psi^brev(k) (forward) or psi^-brev(k) (inverse), with Shoup quotients
    const u32 *perm;                // [n] the inverse of matrix_reps_index_map: NWT_IN_GATHER / NWT_OUT_SCATTER
    u64 q;                          // t
    u64x2 ninv;                     // N^-1 mod t (+Shoup): the last store of the inverse transform
    u32 log_n;
    u32 log_tile, log_cols;         // log_cols == log_tile: a contiguous tile; below: rows of 2^log_cols adjacent columns, 2^lp0 apart
    u32 lp0, stages;                // the pass runs the stages whose pairs are 2^lp0 .. 2^(lp0 + stages - 1) apart
    int in_mode, out_mode;
    u32 values_size;                // NWT_IN_GATHER: slots at or past it are zero
};

// The plan: up to 2^14 words (128 KiB, inside the CU's 160 KiB of LDS) are ONE pass with the whole polynomial in one tile.  A larger
// transform is a contiguous pass (tiles of 2^12 consecutive words: the stages whose pairs are 1 .. 2^11 apart) and a strided pass
// (tiles of n / 2^12 rows of 2^24 / n adjacent columns: the stages whose pairs are 2^12 and more apart; 128 columns = 1 KiB per row at
// n = 2^17); the inverse transform (encode) runs the contiguous pass first, the forward one (decode) the strided pass first.
constexpr u32 kNwtSingleLog = 14, kNwtTileLog = 12, kNwtMaxLog = 2 * kNwtTileLog;
PHA_HD u32 nwt_pass_count(u32 log_n) { return log_n <= kNwtSingleLog ? 1 : 2; }
PHA_HD void nwt_pass_shape(NwtPass &p, u32 log_n, bool inverse, u32 which) {
    p.log_n = log_n;
    if (log_n <= kNwtSingleLog) {
        p.log_tile = p.log_cols = log_n; p.lp0 = 0; p.stages = log_n;
    } else if ((which == 0) == inverse) {
        p.log_tile = p.log_cols = kNwtTileLog; p.lp0 = 0; p.stages = kNwtTileLog;
    } else {
        p.log_tile = kNwtTileLog; p.lp0 = kNwtTileLog; p.stages = log_n - kNwtTileLog; p.log_cols = kNwtTileLog - p.stages;
    }
}

// threads of the workgroup that runs a tile: one unit of 8 words per thread and phase up to 2^13 words, two at 2^14
PHA_HD u32 nwt_threads(u32 log_tile) { return log_tile >= 13 ? 1024u : log_tile >= 9 ? (1u << (log_tile - 3)) : 64u; }

// word of the polynomial behind LDS slot i of tile `tile`
PHA_HD u32 nwt_point(const NwtPass &p, u32 tile, u32 i) {
    if (p.log_cols == p.log_tile) return (tile << p.log_tile) + i;
    return ((i >> p.log_cols) << p.lp0) + (tile << p.log_cols) + (i & ((1u << p.log_cols) - 1));
}

// encode_gpu's load rule (src/batchencoder.cu:55-56): a word with bit 63 set gets + t
PHA_HD u64 batch_sign_rule(u64 v, u64 t) { return v + (v >> 63) * t; }

// first phase: the tile into LDS.  NWT_IN_GATHER is the permutation of encode: word g of the transform's input is slot perm[g] of the
// message (buf[index_map[i]] = v_i read from the other side), zero at or past values_size.  perm is the encoder's own table, so the
// address is below n whatever the message holds.
PHA_HD void nwt_load(const NwtPass &p, u64 *lds, u32 tile, u32 msg, u32 tid, u32 nthreads) {
    const u32 T = 1u << p.log_tile;
    const u64 *in = p.in + (size_t)msg * p.in_stride;
    for (u32 i = tid; i < T; i += nthreads) {
        const u32 g = nwt_point(p, tile, i);
        u64 v;
        if (p.in_mode == NWT_IN_GATHER) {
            const u32 j = p.perm[g];
            v = j < p.values_size ? batch_sign_rule(in[j], p.q) : 0;
        } else {
            v = in[g];
        }
        lds[i] = v;
    }
}

// R consecutive stages of the pass, from its stage s0 up, on every group of 2^R LDS slots they connect: the group sits in
// registers, so R stages cost one LDS round trip.  The butterfly graph is the radix-2 one, stage by stage.
template <int R, bool INV>
PHA_HD void nwt_group(const NwtPass &p, u64 *lds, u32 tile, u32 s0, u32 tid, u32 nthreads) {
    const u32 q = s0 + (p.log_cols == p.log_tile ? 0 : p.log_cols);   // LDS distance (log) of stage s0's pairs
    const u32 units = 1u << (p.log_tile - R);
    const u64 t = p.q, t2 = p.q << 1;
    for (u32 u = tid; u < units; u += nthreads) {
        const u32 base = ((u >> q) << (q + R)) | (u & ((1u << q) - 1));
        u64 x[1 << R];
#pragma unroll
        for (int e = 0; e < (1 << R); e++) x[e] = lds[base + ((u32)e << q)];
#pragma unroll
        for (int k = 0; k < R; k++) {
            const int s = INV ? k : R - 1 - k;   // inverse: pairs grow from stage to stage; forward: they shrink
            const u32 lp = p.lp0 + s0 + s;
#pragma unroll
            for (int e = 0; e < (1 << R); e++) {
                if (e & (1 << s)) continue;
                const u32 grp = nwt_point(p, tile, base + ((u32)e << q)) >> (lp + 1);
                const u64x2 w = p.tw[((1u << p.log_n) >> (lp + 1)) + grp];
                if (INV) gs_bfly(x[e], x[e | (1 << s)], w, t, t2);
                else ct_bfly(x[e], x[e | (1 << s)], w, t, t2);
            }
        }
#pragma unroll
        for (int e = 0; e < (1 << R); e++) lds[base + ((u32)e << q)] = x[e];
    }
}

// one barrier-separated phase of the stages: the next (up to) three of them after `done`; returns how many it ran
template <bool INV>
PHA_HD u32 nwt_stage_phase(const NwtPass &p, u64 *lds, u32 tile, u32 done, u32 tid, u32 nthreads) {
    const u32 r = p.stages - done < 3 ? p.stages - done : 3;
    const u32 s0 = INV ? done : p.stages - done - r;
    if (r == 3) nwt_group<3, INV>(p, lds, tile, s0, tid, nthreads);
    else if (r == 2) nwt_group<2, INV>(p, lds, tile, s0, tid, nthreads);
    else nwt_group<1, INV>(p, lds, tile, s0, tid, nthreads);
    return r;
}

// last phase: the tile out of LDS.  NWT_OUT_LAZY hands the words to the next pass as they are; the other two end the transform with
// the canonical residue (the inverse one times N^-1: one Shoup product reduces any word), NWT_OUT_SCATTER at slot perm[g] (decode:
// out[i] = ntt[index_map[i]] written from the other side).
template <bool INV>
PHA_HD void nwt_store(const NwtPass &p, const u64 *lds, u32 tile, u32 msg, u32 tid, u32 nthreads) {
    const u32 T = 1u << p.log_tile;
    u64 *out = p.out + (size_t)msg * p.out_stride;
    for (u32 i = tid; i < T; i += nthreads) {
        const u32 g = nwt_point(p, tile, i);
        u64 v = lds[i];
        if (p.out_mode == NWT_OUT_LAZY) {
            out[g] = v;
        } else {
            v = INV ? shoup(v, p.ninv, p.q) : csub(csub(v, p.q << 1), p.q);
            out[p.out_mode == NWT_OUT_SCATTER ? p.perm[g] : g] = v;
        }
    }
}

// decode's gather as a pass of its own (decode_gpu, src/batchencoder.cu:91-95): out[i] = src[index_map[i]]
PHA_HD void batch_gather_word(u64 *out, const u64 *src, const u32 *index_map, u32 i) { out[i] = src[index_map[i]]; }
// encode's permutation as a pass of its own (encode_gpu, :51-60, read from the other side so that the stores are consecutive):
// buf[g] = the message's slot perm[g] under the load rule of nwt_load
PHA_HD void batch_permute_word(u64 *buf, const u64 *values, const u32 *perm, u32 values_size, u64 t, u32 g) {
    const u32 j = perm[g];
    buf[g] = j < values_size ? batch_sign_rule(values[j], t) : 0;
}

// matrix_reps_index_map as populate_matrix_reps_index_map builds it (src/batchencoder.cu:25-49): slot i of the first row sits at the
// bit-reversed (5^i - 1) / 2, slot i of the second row at the bit-reversed (2N - 5^i - 1) / 2
PHA_HD u32 batch_brev(u32 x, u32 bits) {
    u32 r = 0;
    for (u32 i = 0; i < bits; i++) r |= ((x >> i) & 1u) << (bits - 1 - i);
    return r;
}
inline void batch_index_map(u32 log_n, u64 *index_map) {
    const size_t slots = (size_t)1 << log_n, row = slots >> 1, m = slots << 1;
    u64 pos = 1;
    for (size_t i = 0; i < row; i++) {
        index_map[i] = batch_brev((u32)((pos - 1) >> 1), log_n);
        index_map[row | i] = batch_brev((u32)((m - pos - 1) >> 1), log_n);
        pos = (pos * 5) & (m - 1);
    }
}

}  // namespace pha
