// tsx_prefilter.h -- counting only the k-mers seen twice (gfx950, wave64): a membership filter that belongs to a map, filled
// in a first pass over the input and consulted by the counting calls in a second one, so that a k-mer that occurs once --
// on real reads most distinct k-mers: sequencing errors -- takes no slot of the table.
//
//   prefilter_windows_kernel   pass 1: the tile front end of sketch_windows_kernel up to the run leaders; a leader ORs the
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
    __shared__ uint64_t s_codes[(TILE + HALO) / 32 + 2];
    __shared__ uint64_t s_nl[(TILE + HALO) / 64 + 3];
    __shared__ uint64_t s_le[TILE / 64];
    __shared__ uint32_t s_lb[TILE / 16];
    __shared__ uint32_t s_wsum[NT / 64];
    __shared__ unsigned long long s_wtot[2][NT / 64];

    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < 3) s_nl[(TILE + HALO) / 64 + tid] = ~0ULL;
    if (tid < 2) s_codes[(TILE + HALO) / 32 + tid] = 0;
    const uint32_t k = (uint32_t)p.k;
    const uint64_t lbase = *line_base;
    const uint64_t need0 = (k >= 64) ? ~0ULL : ((1ULL << k) - 1ULL);
    const uint64_t need1 = (k > 64) ? ((k >= 128) ? ~0ULL : ((1ULL << (k - 64)) - 1ULL)) : 0ULL;
    unsigned long long nvalid = 0;   // valid windows this wave has seen (the same in every lane)
    unsigned long long nagain = 0;   // windows that found their k-mer seen before (per lane: the leaders add their runs)
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t base = tile * TILE;
        lds_barrier();  // previous tile's LDS fully consumed
        {
            const uint64_t off = base + (uint64_t)tid * 16;
            uint32_t nl, le, code;
            const uint4 v = load16(buf, off, n);
            classify16(v, prev_is_nl(buf, off, n, head_open), nl, le, code);
            if constexpr (BR) nl |= rule_bits16<BR>(p, qmap, v, off, n);
            reinterpret_cast<uint32_t *>(s_codes)[tid] = code;
            reinterpret_cast<uint16_t *>(s_nl)[tid] = (uint16_t)nl;
            reinterpret_cast<uint16_t *>(s_le)[tid] = (uint16_t)le;
            if (tid < HALO / 16) {
                const uint64_t hoff = base + TILE + (uint64_t)tid * 16;
                uint32_t hnl, hle, hcode;
                const uint4 hv = load16(buf, hoff, n);
                classify16(hv, false, hnl, hle, hcode);
                if constexpr (BR) hnl |= rule_bits16<BR>(p, qmap, hv, hoff, n);
                reinterpret_cast<uint32_t *>(s_codes)[TILE / 16 + tid] = hcode;
                reinterpret_cast<uint16_t *>(s_nl)[TILE / 16 + tid] = (uint16_t)hnl;
            }
            const uint32_t c = __popc(le);
            const uint32_t inc = wave_incl_scan(c);
            if (lane == 63) s_wsum[tid >> 6] = inc;
            lds_barrier();
            uint32_t woff = tile_line[tile];
            for (int w = 0; w < (tid >> 6); ++w) woff += s_wsum[w];
            s_lb[tid] = woff + inc - c;
        }
        lds_barrier();

        for (int round = 0; round < TILE / BATCH; ++round) {
#pragma unroll
            for (int j = 0; j < PER_THREAD; ++j) {
                const uint32_t pp = (uint32_t)(round * BATCH + j * NT + tid);
                const uint64_t gpos = base + pp;
                const uint32_t grp = pp >> 4;
                const uint32_t le_before = reinterpret_cast<const uint16_t *>(s_le)[grp] & ((1u << (pp & 15)) - 1u);
                const uint32_t line = s_lb[grp] + __popc(le_before);
                const uint32_t w = pp >> 6, o = pp & 63;
                uint64_t m0 = s_nl[w] >> o, m1 = s_nl[w + 1] >> o;
                if (o) { m0 |= s_nl[w + 1] << (64 - o); m1 |= s_nl[w + 2] << (64 - o); }
                const bool valid = (((lbase + line) & p.line_mask) == 1u) && ((m0 & need0) == 0) && ((m1 & need1) == 0) &&
                                   (gpos + k <= n) && (gpos < own_end);
                const unsigned long long vm = __ballot(valid);
                if (vm == 0ULL) continue;
                nvalid += (unsigned long long)__popcll(vm);
                uint64_t x[WK];
                extract_kmer<WK>(s_codes, pp, p.top_mask, x);
                uint64_t xp[WK];
#pragma unroll
                for (int t = 0; t < WK; ++t) xp[t] = __shfl_up((unsigned long long)x[t], 1, 64);
                const bool prev_valid = __shfl_up((int)valid, 1, 64) != 0;
                const bool leader = valid && (lane == 0 || !prev_valid || !kmer_eq<WK>(x, xp));
                // the run a leader stands for, as in count_fastq_kernel: itself and the equal windows in the lanes above
                const unsigned long long bnd = __ballot(leader || !valid);
                const unsigned long long above = (lane == 63) ? 0ULL : (bnd >> (lane + 1));
                const uint32_t runlen = (above ? (uint32_t)__builtin_ctzll(above) : (uint32_t)(63 - lane)) + 1u;
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
