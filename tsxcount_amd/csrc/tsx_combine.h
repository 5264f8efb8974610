// tsx_combine.h -- table set operations (gfx950, wave64): the join of two tables behind tsx_hip_combine
// (include/tsxcount_hip.h; DESIGN.md §3 "Table set operations").
//
// One kernel, combine_sweep_kernel, walks the slots of one table (`src`) in tiles, probes the other (`oth`) for every
// k-mer whose count is in its range, applies the rule and hands on what the rule keeps.  A call sweeps A against B
// (side 0) and, for the per-input totals and for UNION's remainder, B against A (side 1).
//
//   general  (ALIGNED = false)  slot -> k-mer (inverse mapping of src) -> hashed key of oth (forward mapping; CANON:
//            of the pair) -> lookup_key.  Survivors are compacted, one atomic per wave, into a staging chunk of
//            (k-mer, count) that add_kmers_kernel inserts into OUT.
//   aligned  (ALIGNED = true)   src and oth have the same l, slot layout, segment bits and seed: the hashed key read
//            off a slot of src (words_to_key: shifts, no mapping) is oth's key too, and every probe for it stays in the
//            segment of oth that has the number of the segment being walked.  emit = 2 (OUT aligned as well): survivors
//            go straight into OUT by hashed key (insert_key), nothing is staged; emit = 1: the inverse mapping runs
//            for the survivors only.
#pragma once
#include "tsx_kernels.h"

namespace tsx {

constexpr uint32_t CB_TILE = 4 * NT;   // consecutive slots a workgroup walks before it strides on
// Result words of a call (device, summed over every launch of it).
enum CombRes { CB_A_IN = 0, CB_B_IN, CB_BOTH, CB_A_SUM, CB_B_SUM, CB_OUT_N, CB_OUT_SUM, CB_N };

// op / mode: TSX_HIP_OP_* / TSX_HIP_CNT_* of the header.  s_* is the count range of the swept table, o_* of the probed one.
struct CombineArgs {
    int32_t op, mode;
    int32_t side;            // 0: src = A, oth = B;  1: src = B, oth = A
    int32_t emit;            // 0: totals only, 1: stage (k-mer, count), 2: insert into `out` by hashed key (ALIGNED)
    int32_t src_sec, oth_sec;   // the table ever carried: its counts need the secondary array
    uint64_t s_lo, s_hi, o_lo, o_hi;
};

__device__ __forceinline__ uint64_t cb_count(int mode, uint64_t a, uint64_t b) {
    switch (mode) {
        case 0: return a < b ? a : b;
        case 1: return a < b ? b : a;
        case 2: return a + b;
        case 3: return a;
        default: return b;
    }
}

// Slots [slot_lo, slot_hi) of src.  emit = 1: survivors to kmers_out / counts_out at *staged (at most cap; the host
// sizes cap to the slots of the range, so nothing is dropped).  res: CombRes.
template <int WK, bool CANON, bool ALIGNED>
__global__ __launch_bounds__(NT) void combine_sweep_kernel(TableParams src, TableParams oth, TableParams out, CombineArgs a,
                                                           uint64_t slot_lo, uint64_t slot_hi, uint64_t *kmers_out,
                                                           uint64_t *counts_out, uint64_t cap, unsigned long long *staged,
                                                           unsigned long long *res) {
    const int lane = threadIdx.x & 63, W = src.W;
    const uint64_t lt = (1ULL << lane) - 1ULL;
    unsigned long long n_in = 0, n_both = 0, s_sum = 0, o_sum = 0, n_out = 0, out_sum = 0;
    // wave-uniform trip counts: t0 and r are the same for every lane of the workgroup
    for (uint64_t t0 = slot_lo + (uint64_t)blockIdx.x * CB_TILE; t0 < slot_hi; t0 += (uint64_t)gridDim.x * CB_TILE) {
        for (uint32_t r = 0; r < CB_TILE; r += NT) {
            const uint64_t pos = t0 + r + threadIdx.x;
            uint64_t e[4] = {0, 0, 0, 0};
            if (pos < slot_hi) e[0] = src.table[pos * (uint64_t)W];
            uint64_t v[WK], c = 0;   // v: the hashed key (ALIGNED) or the k-mer
            bool keep = false;
            if (e[0] != 0) {
                uint64_t sp = (e[0] >> src.cshift) + (a.src_sec ? sec_get(src, pos) << src.C : 0ULL);
                if (sp < a.s_lo || sp > a.s_hi) sp = 0;
                if (sp) {
                    for (int t = 1; t < W; ++t) e[t] = src.table[pos * (uint64_t)W + t];
                    n_in += 1;
                    const bool probe = a.side == 0 || a.op == 1;
                    uint64_t op = 0;
                    if constexpr (ALIGNED) {
                        words_to_key<WK>(src, pos, e, v);
                        if (probe) op = lookup_key<WK>(oth, v, nullptr, a.oth_sec != 0);
                    } else {
                        words_to_kmer<WK>(src, pos, e, v);
                        if (probe) {
                            uint64_t h[WK];
                            hash_key<CANON, WK>(oth, oth.lut, v, h);
                            op = lookup_key<WK>(oth, h, nullptr, a.oth_sec != 0);
                        }
                    }
                    if (op < a.o_lo || op > a.o_hi) op = 0;
                    const bool both = op != 0;
                    if (a.side == 0) {
                        n_both += both ? 1 : 0;
                        s_sum += both ? sp : 0;
                        o_sum += both ? op : 0;
                        switch (a.op) {
                            case 0: keep = both; c = cb_count(a.mode, sp, op); break;
                            case 1: keep = true; c = both ? cb_count(a.mode, sp, op) : sp; break;
                            case 2: keep = !both; c = sp; break;
                            default: keep = sp > op; c = sp - op; break;
                        }
                    } else {   // what UNION has of B alone (A's sweep wrote the rest)
                        keep = a.op == 1 && !both;
                        c = sp;
                    }
                    n_out += keep ? 1 : 0;
                    out_sum += keep ? c : 0;
                }
            }
            if (a.emit == 2) {
                if constexpr (ALIGNED) { if (keep) insert_key<WK>(out, v, c); }
            } else if (a.emit == 1) {
                const uint64_t bal = __ballot(keep);
                if (bal) {
                    unsigned long long at = 0;
                    if (lane == 0) at = atomicAdd(staged, (unsigned long long)__popcll(bal));
                    at = __shfl(at, 0, 64) + (unsigned long long)__popcll(bal & lt);
                    if (keep && at < cap) {
                        if constexpr (ALIGNED) {
                            uint64_t x[WK];
                            hash_apply<WK>(src, src.ilut, v, x);
#pragma unroll
                            for (int t = 0; t < WK; ++t) kmers_out[at * WK + t] = x[t];
                        } else {
#pragma unroll
                            for (int t = 0; t < WK; ++t) kmers_out[at * WK + t] = v[t];
                        }
                        counts_out[at] = c;
                    }
                }
            }
        }
    }
    for (int d = 32; d > 0; d >>= 1) {
        n_in += __shfl_down(n_in, d, 64); n_both += __shfl_down(n_both, d, 64);
        s_sum += __shfl_down(s_sum, d, 64); o_sum += __shfl_down(o_sum, d, 64);
        n_out += __shfl_down(n_out, d, 64); out_sum += __shfl_down(out_sum, d, 64);
    }
    if (lane == 0) {
        if (n_in) atomicAdd(&res[a.side == 0 ? CB_A_IN : CB_B_IN], n_in);
        if (n_both) atomicAdd(&res[CB_BOTH], n_both);
        if (s_sum) atomicAdd(&res[CB_A_SUM], s_sum);
        if (o_sum) atomicAdd(&res[CB_B_SUM], o_sum);
        if (n_out) atomicAdd(&res[CB_OUT_N], n_out);
        if (out_sum) atomicAdd(&res[CB_OUT_SUM], out_sum);
        if (a.emit == 2 && out_sum) atomicAdd(&out.stats[ST_KMERS], out_sum);
    }
}

}  // namespace tsx
