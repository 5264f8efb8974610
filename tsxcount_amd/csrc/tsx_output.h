// tsx_output.h -- the kernels that take counts out of the table (gfx950, wave64).
//
//   count_histogram_kernel  abundance histogram (jellyfish `histo`): occupied slots per count, streamed
//   format_counts_kernel    the `.count` text of count_kmers.py / main.cpp:224-396: "kmer<TAB>count\n" per k-mer
//
// Both walk a slot range [slot_lo, slot_hi) of the table like dump_kernel (TSXHashMap::getAllKmers,
// TSXHashMap.h:660-722) and leave it unchanged.
#pragma once
#include "tsx_kernels.h"

namespace tsx {

constexpr int HIST_LDS_BINS = 4096;   // bins [0, HIST_LDS_BINS) are summed per workgroup in LDS
constexpr int HIST_UNROLL = 4;        // slots per lane per step of pass A (loads in flight)

// Add `delta` (+1 or -1) per active lane to hist[bin]: lanes that share a bin are folded first (count 1 is nearly
// every k-mer), the leader adds the group's size -- to the workgroup's LDS bin when it has one, else to global memory.
// LDS bins are u32 and may go "negative" in pass B: they are flushed as signed values.
__device__ __forceinline__ void hist_wave_add(bool active, uint64_t bin, int delta, uint32_t *s_bins, uint32_t lds_nb,
                                              unsigned long long *hist) {
    const int lane = threadIdx.x & 63;
    uint64_t todo = __ballot(active);
    while (todo) {
        const int lead = __ffsll((long long)todo) - 1;
        const uint64_t b = __shfl(bin, lead, 64);
        const uint64_t grp = __ballot(active && bin == b);
        if (lane == lead) {
            const uint32_t n = (uint32_t)__popcll(grp);
            if (b < lds_nb) atomicAdd(&s_bins[b], delta > 0 ? n : (uint32_t)(0u - n));
            else atomicAdd(&hist[b], delta > 0 ? (unsigned long long)n : (unsigned long long)(0ULL - n));
        }
        todo &= ~grp;
    }
}

// hist[c] = occupied slots of [slot_lo, slot_hi) whose count is c; hist[nbins - 1] pools every count >= nbins - 1.
// The count of a slot is its in-slot field plus carries << C from the secondary array (slot_to_kmer), taken in two
// streaming passes instead of one secondary probe per slot:
//   pass A  bins the in-slot field f = v >> cshift of word 0 of every occupied slot;
//   pass B  walks the secondary array once: an entry (pos + 1, carry) with pos in the range moves that slot from
//           bin(f) to bin(f + (carry << C)).
// hist must be zero on entry.  The host picks the grid so that no workgroup touches more than 2^31 slots and entries.
__global__ __launch_bounds__(NT) void count_histogram_kernel(TableParams p, uint64_t slot_lo, uint64_t slot_hi,
                                                             uint64_t nbins, unsigned long long *hist) {
    __shared__ uint32_t s_bins[HIST_LDS_BINS];
    const uint32_t lds_nb = (uint32_t)(nbins < (uint64_t)HIST_LDS_BINS ? nbins : (uint64_t)HIST_LDS_BINS);
    for (uint32_t i = threadIdx.x; i < lds_nb; i += NT) s_bins[i] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const uint64_t top = nbins - 1;
    const uint64_t W = (uint64_t)p.W;
    // pass A: wave-uniform trip count, HIST_UNROLL coalesced loads per lane before any binning
    constexpr uint64_t STEP = 64 * HIST_UNROLL;
    const uint64_t nwaves = (uint64_t)gridDim.x * (NT / 64);
    for (uint64_t base = slot_lo + ((uint64_t)blockIdx.x * (NT / 64) + (threadIdx.x >> 6)) * STEP; base < slot_hi;
         base += nwaves * STEP) {
        uint64_t v[HIST_UNROLL];
#pragma unroll
        for (int u = 0; u < HIST_UNROLL; ++u) {
            const uint64_t pos = base + (uint64_t)u * 64 + lane;
            v[u] = pos < slot_hi ? p.table[pos * W] : 0ULL;
        }
#pragma unroll
        for (int u = 0; u < HIST_UNROLL; ++u) {
            const uint64_t f = v[u] >> p.cshift;
            hist_wave_add(v[u] != 0, f < top ? f : top, 1, s_bins, lds_nb, hist);
        }
    }
    // pass B: the secondary array (keyed by slot position + 1, at most one entry per slot)
    const uint64_t sslots = p.sec_mask + 1;
    for (uint64_t i0 = (uint64_t)blockIdx.x * NT + (threadIdx.x & ~63u); i0 < sslots; i0 += (uint64_t)gridDim.x * NT) {
        const uint64_t i = i0 + lane;
        const uint64_t key = i < sslots ? p.sec_keys[i] : 0ULL;
        const uint64_t pos = key - 1;
        uint64_t from = 0, to = 0;
        bool mv = false;
        if (key != 0 && pos >= slot_lo && pos < slot_hi) {
            const uint64_t v = p.table[pos * W];
            if (v != 0) {
                const uint64_t f = v >> p.cshift;
                const uint64_t c = f + (p.sec_cnt[i] << p.C);
                from = f < top ? f : top;
                to = c < top ? c : top;
                mv = from != to;
            }
        }
        if (__ballot(mv)) {
            hist_wave_add(mv, from, -1, s_bins, lds_nb, hist);
            hist_wave_add(mv, to, 1, s_bins, lds_nb, hist);
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < lds_nb; i += NT) {
        const int32_t c = (int32_t)s_bins[i];
        if (c) atomicAdd(&hist[i], (unsigned long long)(long long)c);
    }
}

// v / 10 for every uint64 v: multiply-high by ceil(2^67 / 10), then >> 3.
__device__ __forceinline__ uint64_t div10_u64(uint64_t v) { return __umul64hi(v, 0xCCCCCCCCCCCCCCCDULL) >> 3; }
__device__ __forceinline__ uint32_t dec_digits_u64(uint64_t v) {
    uint32_t d = 1;
    while (v >= 10) { v = div10_u64(v); ++d; }
    return d;
}

// The `.count` text of the slots [slot_lo, slot_hi) whose count c lies in [lower, upper]: one line
// "ACGT...<TAB><decimal c>\n" per k-mer (bases in the order of tsx_hip_decode; CANON: the lexicographically smaller
// strand, as the dumps report it), in no particular order.  Each wave takes its bytes with one atomicAdd on *nbytes and
// its lines with one on *nlines; a wave whose lines would end past `cap` writes nothing, so *nbytes > cap afterwards
// tells the host the text did not fit.
template <int WK, bool CANON = false>
__global__ __launch_bounds__(NT) void format_counts_kernel(TableParams p, uint64_t slot_lo, uint64_t slot_hi, uint64_t lower,
                                                           uint64_t upper, uint8_t *text, uint64_t cap,
                                                           unsigned long long *nbytes, unsigned long long *nlines) {
    const int lane = threadIdx.x & 63;
    const int k = p.k;
    for (uint64_t base = slot_lo + (uint64_t)blockIdx.x * NT + (threadIdx.x & ~63u); base < slot_hi;
         base += (uint64_t)gridDim.x * NT) {
        const uint64_t pos = base + lane;
        const bool occ = pos < slot_hi && p.table[pos * (uint64_t)p.W] != 0;
        uint64_t x[WK], c = 0;
        bool keep = false;
        if (occ) {
            slot_to_kmer<WK>(p, pos, x, c);
            keep = c >= lower && c <= upper;
        }
        const uint64_t kept = __ballot(keep);
        if (!kept) continue;
        if constexpr (CANON) { if (keep) lex_canonical<WK>(x, p.n); }
        const uint32_t nd = keep ? dec_digits_u64(c) : 0u;
        const uint32_t len = keep ? (uint32_t)k + 2u + nd : 0u;
        const uint32_t inc = wave_incl_scan(len);
        const uint32_t total = (uint32_t)__shfl((int)inc, 63, 64);
        unsigned long long at = 0;
        if (lane == 0) {
            at = atomicAdd(nbytes, (unsigned long long)total);
            atomicAdd(nlines, (unsigned long long)__popcll(kept));
        }
        at = __shfl(at, 0, 64);
        if (keep && at + total <= cap) {
            uint8_t *o = text + at + (inc - len);
#pragma unroll
            for (int t = 0; t < WK; ++t) {
                const int b0 = 32 * t, b1 = min(k, 32 * (t + 1));
                for (int b = b0; b < b1; ++b) o[b] = (uint8_t)"ACGT"[(x[t] >> (2 * (b - b0))) & 3];
            }
            o[k] = '\t';
            uint64_t v = c;
            for (int d = (int)nd; d > 0; --d) {
                const uint64_t q = div10_u64(v);
                o[k + d] = (uint8_t)('0' + (uint32_t)(v - q * 10));
                v = q;
            }
            o[k + 1 + nd] = '\n';
        }
    }
}

}  // namespace tsx
