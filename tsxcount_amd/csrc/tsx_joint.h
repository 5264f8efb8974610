// tsx_joint.h -- the joint k-mer spectrum of two tables (gfx950, wave64): the kernel behind tsx_hip_joint_histogram_*
// (include/tsxcount_hip.h; DESIGN.md §3 "Joint spectrum").
//
// matrix[i * nb + j] = distinct k-mers counted i times in A and j times in B (the last bin of each side pools every
// larger count; KAT `comp`).  One kernel, joint_histogram_kernel, sweeps the slots of one table (`src`) in tiles and
// probes the other (`oth`) for every k-mer, exactly as combine_sweep_kernel (tsx_combine.h) does on its general and
// aligned paths; what is new is where the result goes: a cell of the matrix per k-mer instead of six sums per wave.
//   side 0   src = A, oth = B: every k-mer of A is binned at (bin_a(a), bin_b(b)), b = 0 when B lacks it;
//   side 1   src = B, oth = A: only the k-mers A lacks are binned, at (0, bin_b(b)) -- side 0 has binned the rest.
// Real tables put most k-mers into a handful of cells ((1, 0), (0, 1), (1, 1), (c, 1) ...): the lanes of a wave that
// share a cell are folded first and one of them adds the group's size (hist_wave_add of tsx_output.h on the pair), and
// the low corner of the matrix, [0, JH_LDS_A) x [0, JH_LDS_B), is summed per workgroup in LDS and flushed once.
#pragma once
#include "tsx_kernels.h"
#include "tsx_combine.h"

// The corner kept in LDS as u32 (16 KiB at 64 x 64: LDS alone would let ten workgroups share a CU).
#ifndef TSX_JH_LDS_A
#define TSX_JH_LDS_A 64
#endif
#ifndef TSX_JH_LDS_B
#define TSX_JH_LDS_B 64
#endif

namespace tsx {

constexpr uint32_t JH_LDS_A = TSX_JH_LDS_A, JH_LDS_B = TSX_JH_LDS_B;
constexpr uint32_t JH_TILE = CB_TILE;   // consecutive slots a workgroup walks before it strides on

struct JointArgs {
    int32_t side;               // 0: src = A, oth = B;  1: src = B, oth = A
    int32_t src_sec, oth_sec;   // the table ever carried: its counts need the secondary array
};

// One k-mer per active lane into cell (i, j) of the matrix: the lanes of a wave that share a cell are folded, the
// group's leader adds its size -- to the workgroup's LDS corner when the cell lies in it, else to global memory.
__device__ __forceinline__ void joint_wave_add(bool active, uint32_t i, uint32_t j, uint32_t nb, uint32_t *s_corner,
                                               unsigned long long *matrix) {
    const int lane = threadIdx.x & 63;
    const uint32_t cell = i * nb + j;   // < 2^24
    uint64_t todo = __ballot(active);
    while (todo) {
        const int lead = __ffsll((long long)todo) - 1;
        const uint32_t c = (uint32_t)__shfl((int)cell, lead, 64);
        const uint64_t grp = __ballot(active && cell == c);
        if (lane == lead) {
            const uint32_t n = (uint32_t)__popcll(grp);
            if (i < JH_LDS_A && j < JH_LDS_B) atomicAdd(&s_corner[i * JH_LDS_B + j], n);
            else atomicAdd(&matrix[cell], (unsigned long long)n);
        }
        todo &= ~grp;
    }
}

// Slots [slot_lo, slot_hi) of src.  matrix: na x nb uint64, row = bin of the count in A; the caller zeroed it (both
// sides add to it).  The host picks the grid so that no workgroup sweeps 2^31 slots or more: the u32 corner cannot wrap.
template <int WK, bool CANON, bool ALIGNED>
__global__ __launch_bounds__(NT) void joint_histogram_kernel(TableParams src, TableParams oth, JointArgs a, uint64_t slot_lo,
                                                             uint64_t slot_hi, uint32_t na, uint32_t nb,
                                                             unsigned long long *matrix) {
    __shared__ uint32_t s_corner[JH_LDS_A * JH_LDS_B];
    for (uint32_t i = threadIdx.x; i < JH_LDS_A * JH_LDS_B; i += NT) s_corner[i] = 0;
    __syncthreads();
    const int W = src.W;
    const uint64_t top_s = (a.side == 0 ? na : nb) - 1, top_o = (a.side == 0 ? nb : na) - 1;
    // wave-uniform trip counts: t0 and r are the same for every lane of the workgroup
    for (uint64_t t0 = slot_lo + (uint64_t)blockIdx.x * JH_TILE; t0 < slot_hi; t0 += (uint64_t)gridDim.x * JH_TILE) {
        for (uint32_t r = 0; r < JH_TILE; r += NT) {
            const uint64_t pos = t0 + r + threadIdx.x;
            uint64_t e[4] = {0, 0, 0, 0};
            if (pos < slot_hi) e[0] = src.table[pos * (uint64_t)W];
            uint64_t sp = 0, op = 0;
            if (e[0] != 0) sp = (e[0] >> src.cshift) + (a.src_sec ? sec_get(src, pos) << src.C : 0ULL);
            if (sp) {   // (an occupied slot whose count reads 0 holds no k-mer of the table: getKmerCount is 0)
                for (int t = 1; t < W; ++t) e[t] = src.table[pos * (uint64_t)W + t];
                uint64_t v[WK];
                if constexpr (ALIGNED) {
                    words_to_key<WK>(src, pos, e, v);
                    op = lookup_key<WK>(oth, v, nullptr, a.oth_sec != 0);
                } else {
                    uint64_t h[WK];
                    words_to_kmer<WK>(src, pos, e, v);
                    hash_key<CANON, WK>(oth, oth.lut, v, h);
                    op = lookup_key<WK>(oth, h, nullptr, a.oth_sec != 0);
                }
            }
            const uint32_t bs = (uint32_t)(sp < top_s ? sp : top_s), bo = (uint32_t)(op < top_o ? op : top_o);
            if (a.side == 0) joint_wave_add(sp != 0, bs, bo, nb, s_corner, matrix);
            else joint_wave_add(sp != 0 && op == 0, 0u, bs, nb, s_corner, matrix);
        }
    }
    __syncthreads();
    // the corner, clipped to the matrix (cells outside it were never touched)
    for (uint32_t c = threadIdx.x; c < JH_LDS_A * JH_LDS_B; c += NT) {
        const uint32_t n = s_corner[c], i = c / JH_LDS_B, j = c % JH_LDS_B;
        if (n && i < na && j < nb) atomicAdd(&matrix[(uint64_t)i * nb + j], (unsigned long long)n);
    }
}

}  // namespace tsx
