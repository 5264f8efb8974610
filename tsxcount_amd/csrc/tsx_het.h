// tsx_het.h -- heterozygous k-mer pairs of ONE table (gfx950, wave64): the kernel behind tsx_hip_het_histogram_* and
// tsx_hip_het_pairs_device (include/tsxcount_hip.h; DESIGN.md §3 "Heterozygous pairs").
//
// Two k-mers that differ only in their middle base p = (k - 1) / 2 (k odd) are partners (Smudgeplot's hetkmers).  The
// hash is GF(2)-linear with h(0) = 0, so the key of "x with its middle base changed by d" (d = 1..3, XOR on the 2-bit
// code) is key(x) ^ H_d with H_d = A * (d << 2p): three constants per table, made on the host.  het_sweep_kernel sweeps
// the slots in tiles as joint_histogram_kernel (tsx_joint.h) does and probes the SAME table for the three partner keys of
// every in-range slot:
//   not canonical   partner keys s ^ H_d: no decode, no hash;
//   canonical       rc(x ^ (d << 2p)) = rc(x) ^ (d << 2p) (odd k: the middle base stays the middle base and the complement
//                   3 - c commutes with the XOR), so with hr = h(rc x) -- one inverse and one hash per slot -- the
//                   partner keys are min(s ^ H_d, hr ^ H_d).
// A partner key equal to s or to an earlier partner key is dropped (flanks that are reverse complements of each other);
// the in-range survivors found in the table are the slot's family.  The slot OWNS the pair {s, q} when s < q as keys, and
// the family when s is its least key: every pair and every family is counted once.
//   LIST = false   owned pairs go into the matrix [min count][max count] (joint_wave_add: fold, then LDS corner or global
//                  atomic), the five totals are summed per wave and added once per workgroup;
//   LIST = true    owned pairs are compacted into records (wave ballot, one atomic per wave and partner).
#pragma once
#include "tsx_kernels.h"
#include "tsx_joint.h"

namespace tsx {

constexpr uint32_t HET_TILE = CB_TILE;   // consecutive slots a workgroup walks before it strides on

enum HetStatIdx { HS_KMERS = 0, HS_PAIRED = 1, HS_PAIRS = 2, HS_FAM2 = 3, HS_FAM3 = 4, HS_N = 5 };

struct HetArgs {
    uint64_t lower, upper;   // a k-mer counted outside [lower, upper] is absent
    uint64_t hd[3][4];       // H_d = A * (d << 2p), d = 1..3 (limbs >= WK are 0)
    int32_t mode;            // 0: only the pair of a family of exactly two; 1: every pair of every family
    int32_t sec;             // the table ever carried: counts need the secondary array
    int32_t mid_limb, mid_shift;   // the middle base: bits mid_shift, mid_shift + 1 of limb mid_limb of a k-mer
};

// a < b as k-mer texts (A < C < G < T, base 0 first): the first base where they differ decides.
template <int WK>
__device__ __forceinline__ bool kmer_text_less(const uint64_t (&a)[WK], const uint64_t (&b)[WK]) {
    bool decided = false, lt = false;
#pragma unroll
    for (int t = 0; t < WK; ++t) {
        const uint64_t d = a[t] ^ b[t];
        if (!decided && d) {
            const int s = __builtin_ctzll(d) & ~1;
            lt = ((a[t] >> s) & 3ULL) < ((b[t] >> s) & 3ULL);
            decided = true;
        }
    }
    return lt;
}

// Slots [slot_lo, slot_hi).  LIST = false: matrix is n_minor x n_major uint64 and stats HS_N uint64, both zeroed by the
// caller; the host picks the grid so that no workgroup sweeps 2^31 slots or more (the u32 corner and the per-lane sums
// cannot wrap).  LIST = true: records of 2 * WK + 2 uint64 (minor k-mer, major k-mer, minor count, major count) at
// pairs[at * (2 * WK + 2)] for at < cap; *n_pairs counts every owned pair.
template <int WK, bool CANON, bool LIST>
__global__ __launch_bounds__(NT) void het_sweep_kernel(TableParams p, HetArgs a, uint64_t slot_lo, uint64_t slot_hi, uint32_t n_minor,
                                                       uint32_t n_major, unsigned long long *matrix, unsigned long long *stats,
                                                       uint64_t *pairs, uint64_t cap, unsigned long long *n_pairs) {
    __shared__ uint32_t s_corner[LIST ? 1 : JH_LDS_A * JH_LDS_B];
    __shared__ unsigned long long s_stats[HS_N];
    if constexpr (!LIST) {
        for (uint32_t i = threadIdx.x; i < JH_LDS_A * JH_LDS_B; i += NT) s_corner[i] = 0;
        if (threadIdx.x < HS_N) s_stats[threadIdx.x] = 0;
        __syncthreads();
    }
    const int W = p.W;
    const int lane = threadIdx.x & 63;
    const uint64_t lt_mask = (1ULL << lane) - 1ULL;
    uint32_t n_in = 0, n_paired = 0, n_pairs_own = 0, n_f2 = 0, n_f3 = 0;   // per lane: < 2^31 slots a workgroup
    // wave-uniform trip counts: t0 and r are the same for every lane of the workgroup
    for (uint64_t t0 = slot_lo + (uint64_t)blockIdx.x * HET_TILE; t0 < slot_hi; t0 += (uint64_t)gridDim.x * HET_TILE) {
        for (uint32_t r = 0; r < HET_TILE; r += NT) {
            const uint64_t pos = t0 + r + threadIdx.x;
            uint64_t e[4] = {0, 0, 0, 0};
            if (pos < slot_hi) e[0] = p.table[pos * (uint64_t)W];
            uint64_t sp = 0;
            if (e[0] != 0) sp = (e[0] >> p.cshift) + (a.sec ? sec_get(p, pos) << p.C : 0ULL);
            const bool in = sp != 0 && sp >= a.lower && sp <= a.upper;
            uint64_t s[WK], q[3][WK], cq[3] = {0, 0, 0};
            bool own[3] = {false, false, false};
#pragma unroll
            for (int t = 0; t < WK; ++t) s[t] = q[0][t] = q[1][t] = q[2][t] = 0;
            if (in) {
                for (int t = 1; t < W; ++t) e[t] = p.table[pos * (uint64_t)W + t];
                words_to_key<WK>(p, pos, e, s);
                uint64_t hr[WK];
                if constexpr (CANON) {
                    uint64_t x[WK], rx[WK];
                    hash_apply<WK>(p, p.ilut, s, x);
                    revcomp<WK>(x, p.n, rx);
                    hash_apply<WK>(p, p.lut, rx, hr);
                }
                uint32_t members = 0, below = 0;   // in-range partners in the table; those of them with a key below s
#pragma unroll
                for (int d = 0; d < 3; ++d) {
#pragma unroll
                    for (int t = 0; t < WK; ++t) q[d][t] = s[t] ^ a.hd[d][t];
                    if constexpr (CANON) {
                        uint64_t o[WK];
#pragma unroll
                        for (int t = 0; t < WK; ++t) o[t] = hr[t] ^ a.hd[d][t];
                        key_min<WK>(q[d], o);
                    }
                    bool fresh = false;   // differs from s and from every earlier partner key
#pragma unroll
                    for (int t = 0; t < WK; ++t) fresh = fresh || q[d][t] != s[t];
#pragma unroll
                    for (int f = 0; f < d; ++f) {
                        bool ne = false;
#pragma unroll
                        for (int t = 0; t < WK; ++t) ne = ne || q[d][t] != q[f][t];
                        fresh = fresh && ne;
                    }
                    uint64_t c = 0;
                    if (fresh) c = lookup_key<WK>(p, q[d], nullptr, a.sec != 0);
                    if (c < a.lower || c > a.upper) c = 0;
                    cq[d] = c;
                    if (c) {
                        ++members;
                        own[d] = key_less<WK>(s, q[d]);
                        if (!own[d]) ++below;
                    }
                }
                if (a.mode == 0 && members != 1) own[0] = own[1] = own[2] = false;
                if constexpr (!LIST) {
                    ++n_in;
                    n_paired += (a.mode == 0 ? members == 1 : members >= 1) ? 1u : 0u;
                    n_pairs_own += (own[0] ? 1u : 0u) + (own[1] ? 1u : 0u) + (own[2] ? 1u : 0u);
                    n_f2 += (below == 0 && members == 1) ? 1u : 0u;
                    n_f3 += (below == 0 && members >= 2) ? 1u : 0u;
                }
            }
            if constexpr (!LIST) {
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    const uint64_t lo = sp < cq[d] ? sp : cq[d], hi = sp < cq[d] ? cq[d] : sp;
                    const uint32_t bi = (uint32_t)(lo < n_minor - 1 ? lo : n_minor - 1), bj = (uint32_t)(hi < n_major - 1 ? hi : n_major - 1);
                    joint_wave_add(own[d], bi, bj, n_major, s_corner, matrix);
                }
            } else {
                const bool any = own[0] || own[1] || own[2];
                uint64_t x[WK], xs[WK];   // the k-mer of the slot, and as a dump reports it
#pragma unroll
                for (int t = 0; t < WK; ++t) x[t] = xs[t] = 0;
                if (any) {
                    hash_apply<WK>(p, p.ilut, s, x);
#pragma unroll
                    for (int t = 0; t < WK; ++t) xs[t] = x[t];
                    if constexpr (CANON) lex_canonical<WK>(xs, p.n);
                }
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    const uint64_t grp = __ballot(own[d]);
                    if (grp == 0) continue;   // (wave-uniform)
                    const int lead = __ffsll((long long)grp) - 1;
                    unsigned long long at = 0;
                    if (lane == lead) at = atomicAdd(n_pairs, (unsigned long long)__popcll(grp));
                    at = __shfl(at, lead, 64) + (unsigned long long)__popcll(grp & lt_mask);
                    if (own[d] && at < cap) {
                        uint64_t y[WK];
#pragma unroll
                        for (int t = 0; t < WK; ++t) y[t] = x[t] ^ (t == a.mid_limb ? (uint64_t)(d + 1) << a.mid_shift : 0ULL);
                        if constexpr (CANON) lex_canonical<WK>(y, p.n);
                        const bool slot_minor = sp < cq[d] || (sp == cq[d] && kmer_text_less<WK>(xs, y));
                        uint64_t *rec = pairs + at * (uint64_t)(2 * WK + 2);
#pragma unroll
                        for (int t = 0; t < WK; ++t) {
                            rec[t] = slot_minor ? xs[t] : y[t];
                            rec[WK + t] = slot_minor ? y[t] : xs[t];
                        }
                        rec[2 * WK] = slot_minor ? sp : cq[d];
                        rec[2 * WK + 1] = slot_minor ? cq[d] : sp;
                    }
                }
            }
        }
    }
    if constexpr (!LIST) {
        unsigned long long v[HS_N] = {n_in, n_paired, n_pairs_own, n_f2, n_f3};
#pragma unroll
        for (int i = 0; i < HS_N; ++i) {
            for (int d = 32; d > 0; d >>= 1) v[i] += __shfl_down(v[i], d, 64);
            if (lane == 0 && v[i]) atomicAdd(&s_stats[i], v[i]);
        }
        __syncthreads();
        if (threadIdx.x < HS_N && s_stats[threadIdx.x]) atomicAdd(&stats[threadIdx.x], s_stats[threadIdx.x]);
        // the corner, clipped to the matrix (cells outside it were never touched)
        for (uint32_t c = threadIdx.x; c < JH_LDS_A * JH_LDS_B; c += NT) {
            const uint32_t n = s_corner[c], i = c / JH_LDS_B, j = c % JH_LDS_B;
            if (n && i < n_minor && j < n_major) atomicAdd(&matrix[(uint64_t)i * n_major + j], (unsigned long long)n);
        }
    }
}

}  // namespace tsx
