// tsx_prefilter.h -- counting only the k-mers seen twice (gfx950, wave64): a membership filter that belongs to a map, filled
// in a first pass over the input and consulted by the counting calls in a second one, so that a k-mer that occurs once --
// on real reads most distinct k-mers: sequencing errors -- takes no slot of the table.
//
//   prefilter_windows_kernel   pass 1: the tile front end (tsx_kernels.h) up to the run lengths; a leader ORs the
//                              mask of its k-mer into filter A ("seen") and, when A already held it or the run has
//                              followers, into filter B ("seen again").  Adds its exact totals: windows seen, windows
//                              that found their k-mer seen before.
//   count_fastq_kernel<.., PF> pass 2 (tsx_kernels.h): a leader whose mask is not in B inserts nothing.
//   prefilter_fill_kernel      the set bits of A and B
//
// The element and its hash are the sketch's (tsx_device.h: sketch_hash): the k-mer in the tsx_hip_encode layout, on a
// canonical map its lexicographically smaller strand -- the filters depend on neither l, s nor the seed.  Words and mask:
// pf_word_a, pf_word_b, pf_mask (tsx_device.h).  One key touches one 64-bit word per filter.
//
// THE CONTRACT.  An occurrence of a k-mer that is not the first to reach A finds the whole mask there (bits are only ever
// set, and the returning atomic orders the occurrences of one word), so after pass 1 the mask of every k-mer that occurs
// twice is in B, and pass 2 inserts EVERY occurrence of such a k-mer: it is in the table with its exact count.  A k-mer
// that occurs once is in B only when other keys set its bits (a false positive): it is then in the table with count 1.
// The false-positive rate decides how many slots are saved, never whether a count is right.
// B is read by pass 2 only after every pass-1 kernel has finished (the same stream, or an event): no flags, no fences.
#pragma once
#include "tsx_sketch.h"

namespace tsx {

// Words of the totals a map keeps for its prefilter (device memory, added to by the kernels).
enum PfTotal { PF_SEEN = 0, PF_AGAIN = 1, PF_ADMITTED = 2, PF_SKIPPED = 3, PF_SET_A = 4, PF_SET_B = 5, PF_NTOT = 8 };

// The start positions [0, min(own_end, n)) of buf, as sketch_windows_kernel walks them.  fa, fb: the filters; tot: the
// map's totals.  A plain load in front of either atomic skips it when the mask is already there.
template <int WK, bool CANON = false, bool BR = false>
__global__ __launch_bounds__(NT, 2) void prefilter_windows_kernel(TableParams p, const uint8_t *buf, uint64_t n, uint64_t own_end,
                                                                  int head_open, const uint32_t *tile_line, uint64_t ntiles,
                                                                  const unsigned long long *line_base, int bits,
                                                                  unsigned long long *fa, unsigned long long *fb,
                                                                  unsigned long long *tot,
                                                                  const uint16_t *qmap = nullptr) {
    __shared__ TileLds<uint32_t> s;
    __shared__ unsigned long long s_wtot[2][NT / 64];

    const int tid = threadIdx.x, lane = tid & 63;
    s.set_sentinels(tid);
    const WindowRule rule(p, n, own_end, *line_base);
    unsigned long long nvalid = 0;   // valid windows this wave has seen (the same in every lane)
    unsigned long long nagain = 0;   // windows that found their k-mer seen before (per lane: the leaders add their runs)
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t base = tile * TILE;
        lds_barrier();  // previous tile's LDS fully consumed
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
                const bool leader = run_leader<WK>(x, valid, lane);
                // the run a leader stands for, as in count_fastq_kernel: itself and the equal windows in the lanes above
                const uint32_t runlen = run_length(leader, valid, lane);
                if (leader) {
                    if constexpr (CANON) lex_canonical<WK>(x, p.n);
                    const uint64_t v = sketch_hash<WK>(x), mask = pf_mask(v);
                    unsigned long long *const wa = fa + pf_word_a(v, bits), *const wb = fb + pf_word_b(v, bits);
                    // Bits are only ever set: a stale read can only miss some, and then costs an atomic too many --
                    // never a wrong answer.  A read that shows the mask is true for good.
                    unsigned long long old = __hip_atomic_load(wa, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if ((old & mask) != mask) old = atomicOr(wa, (unsigned long long)mask);
                    const bool seen = (old & mask) == mask;
                    nagain += seen ? runlen : runlen - 1u;
                    // a run with followers has been seen twice by that alone, whatever A said
                    if (seen || runlen > 1u) {
                        const unsigned long long cur = __hip_atomic_load(wb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if ((cur & mask) != mask) atomicOr(wb, (unsigned long long)mask);
                    }
                }
            }
        }
    }
    for (int d = 32; d > 0; d >>= 1) nagain += __shfl_down(nagain, d, 64);
    if (lane == 0) { s_wtot[0][tid >> 6] = nvalid; s_wtot[1][tid >> 6] = nagain; }
    __syncthreads();
    if (tid < 2) {
        unsigned long long t = 0;
        for (int w = 0; w < NT / 64; ++w) t += s_wtot[tid][w];
        if (t) atomicAdd(tot + (tid == 0 ? PF_SEEN : PF_AGAIN), t);
    }
}

// tot[PF_SET_A] += the set bits of fa[0, na), tot[PF_SET_B] += those of fb[0, nb)
__global__ __launch_bounds__(NT) void prefilter_fill_kernel(const unsigned long long *fa, uint64_t na,
                                                            const unsigned long long *fb, uint64_t nb, unsigned long long *tot) {
    unsigned long long ca = 0, cb = 0;
    const uint64_t stride = (uint64_t)gridDim.x * NT;
    for (uint64_t i = (uint64_t)blockIdx.x * NT + threadIdx.x; i < na; i += stride) ca += (unsigned long long)__popcll(fa[i]);
    for (uint64_t i = (uint64_t)blockIdx.x * NT + threadIdx.x; i < nb; i += stride) cb += (unsigned long long)__popcll(fb[i]);
    for (int d = 32; d > 0; d >>= 1) { ca += __shfl_down(ca, d, 64); cb += __shfl_down(cb, d, 64); }
    if ((threadIdx.x & 63) == 0) {
        if (ca) atomicAdd(tot + PF_SET_A, ca);
        if (cb) atomicAdd(tot + PF_SET_B, cb);
    }
}

}  // namespace tsx
