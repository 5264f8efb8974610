// tsx_sketch.h -- table sizing (gfx950, wave64): a HyperLogLog sketch of the k-mers a text would put into a table, so
// that the slot count can be chosen before anything is counted.
//
//   sketch_windows_kernel      the tile front end (tsx_kernels.h) up to the run leaders; then, instead of a table
//                              lookup, the k-mer (its lexicographically smaller strand on a canonical map) is hashed and
//                              raises one of 2^p registers kept in LDS.  Every workgroup folds its registers into the
//                              global ones when it ends, and adds its exact number of valid windows.
//   sketch_records_kernel      the record count of a device text (device_windows leaves it on the device) into the totals
//
// The element is the k-mer in the tsx_hip_encode layout, NOT the table's GF(2) key: the registers depend on neither l, s
// nor the seed, and the host functions (tsxcount_hip.hip: tsx_hip_sketch_kmers_host) compute the same ones without a GPU.
//   v = 0x9E3779B97F4A7C15;  for t in 0 .. WK-1: v = mix64(v ^ x[t])
//   idx = v >> (64 - p),  rank = 1 + clz((v << p) | 1 << (p - 1)),  M[idx] = max(M[idx], rank)
// max commutes: the registers depend on neither the grid, the pieces, the windows nor the order of anything.
#pragma once
#include "tsx_median.h"

namespace tsx {

constexpr int SKETCH_P_MIN = 10, SKETCH_P_MAX = 14;

// (sketch_hash: tsx_device.h -- the prefilter consulted by count_fastq_kernel hashes the same element)
// The register a hash raises and the rank it raises it to (1 .. 64 - p + 1).
__host__ __device__ __forceinline__ void sketch_slot(uint64_t v, int prec, uint32_t &idx, uint32_t &rank) {
    idx = (uint32_t)(v >> (64 - prec));
    rank = 1u + (uint32_t)__builtin_clzll((v << prec) | (1ULL << (prec - 1)));
}

// The start positions [0, min(own_end, n)) of buf, as window_counts_kernel walks them.  regs: 2^prec global registers,
// max-combined into; *kmers: the valid windows, added to.  Dynamic LDS: 4 << prec bytes (the workgroup's registers).
template <int WK, bool CANON = false, bool BR = false>
__global__ __launch_bounds__(NT, 2) void sketch_windows_kernel(TableParams p, const uint8_t *buf, uint64_t n, uint64_t own_end,
                                                               int head_open, const uint32_t *tile_line, uint64_t ntiles,
                                                               const unsigned long long *line_base, int prec, uint32_t *regs,
                                                               unsigned long long *kmers, const uint16_t *qmap = nullptr) {
    __shared__ TileLds<uint32_t> s;
    __shared__ unsigned long long s_wvalid[NT / 64];
    extern __shared__ uint64_t s_dyn[];
    uint32_t *const s_reg = reinterpret_cast<uint32_t *>(s_dyn);

    const int tid = threadIdx.x, lane = tid & 63;
    const uint32_t nreg = 1u << prec;
    for (uint32_t i = tid; i < nreg; i += NT) s_reg[i] = 0;
    s.set_sentinels(tid);
    const WindowRule rule(p, n, own_end, *line_base);
    unsigned long long nvalid = 0;   // valid windows this wave has seen (the same in every lane)
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t base = tile * TILE;
        lds_barrier();  // previous tile's LDS fully consumed (the first tile: the registers are zero)
        tile_stage<BR>(s, tile_load(buf, n, head_open, tile_line, tile, tid), p, qmap, base, n, tid);
        lds_barrier();

        for (int round = 0; round < TILE / BATCH; ++round) {
#pragma unroll
            for (int j = 0; j < PER_THREAD; ++j) {
                const uint32_t pp = (uint32_t)(round * BATCH + j * NT + tid);
                uint32_t line;
                const bool valid = window_valid(s, rule, base, pp, line);
                const unsigned long long vm = __ballot(valid);
                if (vm == 0ULL) continue;
                nvalid += (unsigned long long)__popcll(vm);
                uint64_t x[WK];
                extract_kmer<WK>(s.codes, pp, p.top_mask, x);
                // a window equal to the one in the lane below has its hash: leaders only
                const bool leader = run_leader<WK>(x, valid, lane);
                if (leader) {
                    if constexpr (CANON) lex_canonical<WK>(x, p.n);
                    uint32_t idx, rank;
                    sketch_slot(sketch_hash<WK>(x), prec, idx, rank);
                    // (once the registers are warm almost no update raises one: the read keeps the atomics rare)
                    if (rank > s_reg[idx]) atomicMax(&s_reg[idx], rank);
                }
            }
        }
    }
    if (lane == 0) s_wvalid[tid >> 6] = nvalid;
    __syncthreads();   // every wave's updates and count are in LDS
    for (uint32_t i = tid; i < nreg; i += NT) {
        const uint32_t r = s_reg[i];
        // (a stale read is a smaller one: an atomic too many, never one too few)
        if (r && r > __hip_atomic_load(regs + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(regs + i, r);
    }
    if (tid == 0) {
        unsigned long long t = 0;
        for (int w = 0; w < NT / 64; ++w) t += s_wvalid[w];
        if (t) atomicAdd(kmers, t);
    }
}

// totals[1] += *nrec
__global__ void sketch_records_kernel(const unsigned long long *nrec, unsigned long long *totals) {
    if (threadIdx.x == 0 && blockIdx.x == 0) totals[1] += *nrec;
}

}  // namespace tsx
