// tsx_bin.h -- read binning by two tables (gfx950, wave64): one scan of the text, hits in A and in B per record.
//
//   bin_reads_kernel   the tile front end and the lookup schedule of query_reads_kernel with TWO tables: a leader hashes
//                      its k-mer for A and for B and issues the first probe load of both before any is waited for (16
//                      random HBM loads in flight per lane); a segmented per-record reduction of three hit counts ends
//                      in at most four global atomics per (wave, record) run
//   bin_class_kernel   the class of every record from its stats and the rule, and the four class counters
//   bin_len_kernel     the bytes a record contributes to the output of one class (filter_len_kernel's part); the u64
//                      scan kernels and filter_copy_kernel of tsx_query.h do the rest, once per output
//
// Stats layout: four uint64 per record {kmers, hits_a, hits_b, hits_both} (tsx_hip_bin_stats).
#pragma once
#include "tsx_query.h"

namespace tsx {

enum { BS_KMERS = 0, BS_A = 1, BS_B = 2, BS_BOTH = 3, BS_N = 4 };
enum { BIN_CLASS_A = 0, BIN_CLASS_B = 1, BIN_CLASS_AMBIGUOUS = 2, BIN_CLASS_NONE = 3 };

// The count ranges of a hit, lower bounds already >= 1.
struct BinRanges {
    uint64_t a_lower, a_upper, b_lower, b_upper;
};

// How a launch gets B's hashed keys:
//   BIN_ONE_LUT    A and B hash alike (one seed): one LUT in LDS, one hash, the key serves both tables
//   BIN_TWO_LUT    two LUTs, two hashes; both keys of every position live from the issue to the count (no instantiation
//                  spills: profiles/bin_resources.txt)
enum { BIN_ONE_LUT = 0, BIN_TWO_LUT = 1 };

// A round of BATCH start positions (ProbeRound of tsx_query.h for two tables).
template <int WK, int FORM>
struct BinRound {
    static constexpr bool KEEP_B = FORM == BIN_TWO_LUT;
    uint64_t hk[PER_THREAD][WK];                                 // A's keys (BIN_ONE_LUT: B's too)
    uint64_t hb[KEEP_B ? PER_THREAD : 1][KEEP_B ? WK : 1];       // B's keys, where they are kept
    uint64_t va[PER_THREAD], vb[PER_THREAD];                     // the first probe of each table
    uint32_t vbits, lbits;
};

// probe_round_issue for two tables: every first probe load of the lane, A's and B's, before any is waited for.
template <bool CANON, int WK, int FORM>
__device__ __forceinline__ void bin_round_issue(const TableParams &pa, const TableParams &pb, const uint64_t *lut_a,
                                                const uint64_t *lut_b, const TileLds<uint32_t> &s, const WindowRule &rule,
                                                uint64_t base, int round, int tid, BinRound<WK, FORM> &br) {
    br.vbits = 0; br.lbits = 0;
#pragma unroll
    for (int j = 0; j < PER_THREAD; ++j) {
        const uint32_t pp = (uint32_t)(round * BATCH + j * NT + tid);
        uint32_t line;
        const bool valid = window_valid(s, rule, base, pp, line);
        br.va[j] = 0; br.vb[j] = 0;
        if (__ballot(valid) == 0ULL) continue;
        uint64_t x[WK];
        extract_kmer<WK>(s.codes, pp, pa.top_mask, x);
        const bool leader = run_leader<WK>(x, valid, tid & 63);
        br.vbits |= valid ? (1u << j) : 0u;
        br.lbits |= leader ? (1u << j) : 0u;
        if (leader) {
            hash_key<CANON, WK>(pa, lut_a, x, br.hk[j]);
            br.va[j] = first_probe<WK>(pa, br.hk[j]);
            if constexpr (FORM == BIN_ONE_LUT) {
                br.vb[j] = first_probe<WK>(pb, br.hk[j]);
            } else {
                hash_key<CANON, WK>(pb, lut_b, x, br.hb[j]);
                br.vb[j] = first_probe<WK>(pb, br.hb[j]);
            }
        }
    }
}

// probe_round_count for two tables: position j of the round.  Returns the ballot of the valid lanes; when it is not
// empty, bit 0 of `hit` says a(x) is in A's range and bit 1 that b(x) is in B's, for every valid lane: leaders finish
// both probes, followers take the two bits of the nearest leader at or below them by ONE shuffle (the counts themselves
// are not needed past the range tests).  Called by whole waves.
template <int WK, int FORM>
__device__ __forceinline__ unsigned long long bin_round_count(const TableParams &pa, const TableParams &pb, const BinRanges &rg,
                                                              const BinRound<WK, FORM> &br, int j, int lane, uint32_t &hit) {
    const bool valid = (br.vbits >> j) & 1u, leader = (br.lbits >> j) & 1u;
    const unsigned long long vmask = __ballot(valid);
    hit = 0;
    if (vmask == 0ULL) return vmask;
    if (leader) {
        const uint64_t ca = lookup_rest<WK>(pa, br.hk[j], br.va[j]);
        uint64_t cb;
        if constexpr (FORM == BIN_ONE_LUT) cb = lookup_rest<WK>(pb, br.hk[j], br.vb[j]);
        else cb = lookup_rest<WK>(pb, br.hb[j], br.vb[j]);
        hit = ((ca >= rg.a_lower && ca <= rg.a_upper) ? 1u : 0u) | ((cb >= rg.b_lower && cb <= rg.b_upper) ? 2u : 0u);
    }
    const unsigned long long lmask = __ballot(leader) & (~0ULL >> (63 - lane));   // leaders at or below the lane
    const int src = lmask ? 63 - __builtin_clzll(lmask) : lane;
    hit = (uint32_t)__shfl((int)hit, src, 64);
    return vmask;
}

// query_reads_kernel with two tables.  pa also carries what the front end reads (k, the record rule, the base rule): the
// entry points refuse tables that differ in them.  Dynamic LDS: A's LUT, then B's unless FORM is BIN_ONE_LUT.
// stats[r] is written for r < cap only; nothing else is written, the tables are only read.
template <int WK, bool CANON = false, bool BR = false, int FORM = BIN_ONE_LUT>
__global__ __launch_bounds__(NT, 2) void bin_reads_kernel(TableParams pa, TableParams pb, const uint8_t *buf, uint64_t n,
                                                          uint64_t own_end, int head_open, const uint32_t *tile_line,
                                                          uint64_t ntiles, const unsigned long long *line_base, uint32_t lshift,
                                                          BinRanges rg, unsigned long long *stats, uint64_t cap,
                                                          const uint16_t *qmap = nullptr) {
    __shared__ TileLds<uint32_t> s;
    extern __shared__ uint64_t s_lut[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int lut_words = pa.groups * (1 << pa.g) * WK;
    for (int i = tid; i < lut_words; i += NT) s_lut[i] = pa.lut[i];
    if constexpr (FORM != BIN_ONE_LUT)
        for (int i = tid; i < lut_words; i += NT) s_lut[lut_words + i] = pb.lut[i];
    const uint64_t *lut_a = (const uint64_t *)s_lut, *lut_b = lut_a + (FORM != BIN_ONE_LUT ? lut_words : 0);
    s.set_sentinels(tid);
    const WindowRule rule(pa, n, own_end, *line_base);
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t base = tile * TILE;
        lds_barrier();  // previous tile's LDS fully consumed
        tile_stage<BR>(s, tile_load(buf, n, head_open, tile_line, tile, tid), pa, qmap, base, n, tid);
        lds_barrier();

        for (int round = 0; round < TILE / BATCH; ++round) {
            BinRound<WK, FORM> br;
            bin_round_issue<CANON, WK, FORM>(pa, pb, lut_a, lut_b, s, rule, base, round, tid, br);
#pragma unroll
            for (int j = 0; j < PER_THREAD; ++j) {
                const bool valid = (br.vbits >> j) & 1u;
                uint32_t hit;
                const unsigned long long vmask = bin_round_count<WK, FORM>(pa, pb, rg, br, j, lane, hit);
                if (vmask == 0ULL) continue;
                // runs of valid lanes, one per record (query_reads_kernel); three hit counts ride the reduction
                const bool head = valid && (lane == 0 || !((vmask >> (lane - 1)) & 1ULL));
                const uint32_t seg = run_length(head, valid, lane);
                uint32_t ha = (valid && (hit & 1u)) ? 1u : 0u, hb = (valid && (hit & 2u)) ? 1u : 0u;
                uint32_t hab = (valid && hit == 3u) ? 1u : 0u;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const uint32_t oa = __shfl_down(ha, d, 64), ob = __shfl_down(hb, d, 64), oab = __shfl_down(hab, d, 64);
                    if ((uint32_t)d < seg) { ha += oa; hb += ob; hab += oab; }
                }
                if (head) {
                    const uint32_t line = tile_line_of(s, (uint32_t)(round * BATCH + j * NT + tid));
                    const uint64_t rec = (rule.lbase + line) >> lshift;
                    if (rec < cap) {
                        unsigned long long *st = stats + rec * BS_N;
                        atomicAdd(st + BS_KMERS, (unsigned long long)seg);
                        if (ha) atomicAdd(st + BS_A, (unsigned long long)ha);
                        if (hb) atomicAdd(st + BS_B, (unsigned long long)hb);
                        if (hab) atomicAdd(st + BS_BOTH, (unsigned long long)hab);
                    }
                }
            }
        }
    }
}

// The class rule (tsx_hip_bin_rule): q = hits >= min_hits; a side wins when it qualifies, has more hits than the other
// and hits * 1000 >= ratio_milli * the other's (a sequence line is shorter than 4 GiB and ratio_milli <= 10^6: 64 bits).
__host__ __device__ __forceinline__ uint32_t bin_class_of(uint64_t ha, uint64_t hb, uint64_t min_hits, uint64_t ratio_milli) {
    const bool qa = ha >= min_hits, qb = hb >= min_hits;
    if (qa && ha > hb && ha * 1000ULL >= ratio_milli * hb) return BIN_CLASS_A;
    if (qb && hb > ha && hb * 1000ULL >= ratio_milli * ha) return BIN_CLASS_B;
    return (qa || qb) ? BIN_CLASS_AMBIGUOUS : BIN_CLASS_NONE;
}

// cls[r] for records [0, nrec); count[c] += the records of class c (one atomic per wave and class that occurs).
__global__ __launch_bounds__(NT) void bin_class_kernel(const unsigned long long *stats, uint64_t nrec, uint64_t min_hits,
                                                       uint32_t ratio_milli, uint8_t *cls, unsigned long long *count) {
    const int lane = threadIdx.x & 63;
    const uint64_t stride = (uint64_t)gridDim.x * NT;
    for (uint64_t r0 = (uint64_t)blockIdx.x * NT; r0 < nrec; r0 += stride) {   // (whole waves stay in the loop: ballots)
        const uint64_t r = r0 + threadIdx.x;
        uint32_t c = 4;
        if (r < nrec) {
            c = bin_class_of(stats[r * BS_N + BS_A], stats[r * BS_N + BS_B], min_hits, ratio_milli);
            cls[r] = (uint8_t)c;
        }
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            const unsigned long long m = __ballot(c == k);
            if (lane == 0 && m) atomicAdd(count + k, (unsigned long long)__popcll(m));
        }
    }
}

// len[r] = the bytes record r contributes to the output of class `wanted`: its span, plus the '\n' the text lacks for the
// last record when nl_last; 0 for the records of the other classes.
__global__ __launch_bounds__(NT) void bin_len_kernel(const uint8_t *cls, const unsigned long long *span, uint64_t nrec,
                                                     uint32_t wanted, int nl_last, unsigned long long *len) {
    for (uint64_t r = (uint64_t)blockIdx.x * NT + threadIdx.x; r < nrec; r += (uint64_t)gridDim.x * NT)
        len[r] = cls[r] == wanted ? span[r * 2 + 1] - span[r * 2] + ((nl_last && r + 1 == nrec) ? 1 : 0) : 0;
}

}  // namespace tsx
