// tsx_median.h -- the median k-mer abundance of reads (gfx950, wave64): the count of every window of a text, the
// median of every record's counts, and the filter on it.
//
//   window_counts_kernel       the tile front end (tsx_kernels.h) and the lookup schedule (tsx_query.h); then one
//                              uint32 per start position: min(c, 0xFFFFFFFE) for a k-mer under the base rule, else
//                              TSX_HIP_NO_KMER (a coalesced 256-byte store per wave and position group)
//   median_select_kernel       one wave per record: radix select of rank m / 2 among the record's profile entries, most
//                              significant byte first; records with a long sequence line go to a list instead
//   median_select_long_kernel  one workgroup per record of that list: the same select, the profile streamed with
//                              16-byte loads into one LDS histogram per wave
//   median_len_kernel          filter_len_kernel with the median rule
// The profile of a record is contiguous (its sequence line), so no selection combines anything across workgroups.
//
// Medians layout: two uint64 per record {kmers, median} (tsx_hip_read_median).
#pragma once
#include "tsx_trim.h"

namespace tsx {

constexpr uint32_t NO_KMER = 0xFFFFFFFFu;   // TSX_HIP_NO_KMER
constexpr int MED_REG = 8;                  // profile entries a lane of the wave form keeps in registers

// solid_bits_kernel with the count kept: profile[i] for the start positions i < min(own_end, n) of buf -- `profile` is
// the entry of position 0 of buf.  Every entry is written once, by the window that owns it; nothing at or past n.
// The tiles [tile0, ntiles) only: the whole text passes 0, a round of the normalization (tsx_normalize.h) its own range.
template <int WK, bool CANON = false, bool BR = false>
__global__ __launch_bounds__(NT, 2) void window_counts_kernel(TableParams p, const uint8_t *buf, uint64_t n, uint64_t own_end,
                                                              int head_open, const uint32_t *tile_line, uint64_t tile0,
                                                              uint64_t ntiles, const unsigned long long *line_base, uint32_t *profile,
                                                              const uint16_t *qmap = nullptr) {
    __shared__ TileLds<uint32_t> s;
    extern __shared__ uint64_t s_lut[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int lut_words = p.groups * (1 << p.g) * WK;
    for (int i = tid; i < lut_words; i += NT) s_lut[i] = p.lut[i];
    s.set_sentinels(tid);
    const WindowRule rule(p, n, own_end, *line_base);
    const uint64_t wr_end = min(own_end, n);
    for (uint64_t tile = tile0 + blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t base = tile * TILE;
        lds_barrier();  // previous tile's LDS fully consumed
        tile_stage<BR>(s, tile_load(buf, n, head_open, tile_line, tile, tid), p, qmap, base, n, tid);
        lds_barrier();

        for (int round = 0; round < TILE / BATCH; ++round) {
            ProbeRound<WK> pr;
            probe_round_issue<CANON, WK>(p, (const uint64_t *)s_lut, s, rule, base, round, tid, pr);
#pragma unroll
            for (int j = 0; j < PER_THREAD; ++j) {
                const bool valid = (pr.vbits >> j) & 1u;
                uint64_t c;
                uint32_t out = NO_KMER;
                if (probe_round_count<WK>(p, pr, j, lane, c) != 0ULL && valid) out = (uint32_t)min(c, (uint64_t)(NO_KMER - 1u));
                const uint64_t gpos = base + (uint64_t)(round * BATCH + j * NT + tid);
                if (gpos < wr_end) profile[gpos] = out;
            }
        }
    }
}

// One more entry for a 256-bin histogram: lanes that hold a candidate of the bin of the wave's first candidate add once,
// together (the counts of a read share their high bytes, and mostly the low one); the others add one each.  Called by
// whole waves.
__device__ __forceinline__ void hist_add(uint32_t *h, bool cand, uint32_t bin, int lane) {
    const unsigned long long cm = __ballot(cand);
    if (cm == 0ULL) return;
    const int first = __builtin_ctzll(cm);
    const uint32_t b0 = (uint32_t)__shfl((int)bin, first, 64);
    const unsigned long long same = __ballot(cand && bin == b0);
    if (lane == first) atomicAdd(h + b0, (uint32_t)__popcll(same));
    if (cand && bin != b0) atomicAdd(h + bin, 1u);
}

// The bin of h[0..256) that holds rank `rank` (counting from 0 through the bins in order), and the rank inside it; the
// sum of all bins in `total`.  first: rank = total / 2 (the histogram of all values counts them).  Every lane of the wave
// gets the same answer; total = 0 gives bin 0.  Lane i scans bins 4 i .. 4 i + 3.
__device__ __forceinline__ void scan_bins(const uint32_t *h, int lane, bool first, uint32_t &rank, uint32_t &bin,
                                          uint32_t &total) {
    const uint4 q = reinterpret_cast<const uint4 *>(h)[lane];
    const uint32_t t = q.x + q.y + q.z + q.w;
    const uint32_t inc = wave_incl_scan(t), exc = inc - t;
    total = (uint32_t)__shfl((int)inc, 63, 64);
    if (first) rank = total / 2;
    const unsigned long long hm = __ballot(rank >= exc && rank < inc);
    const int src = hm ? __builtin_ctzll(hm) : 0;
    uint32_t r = rank - exc, b = (uint32_t)lane * 4;
    if (r >= q.x) {
        r -= q.x; ++b;
        if (r >= q.y) {
            r -= q.y; ++b;
            if (r >= q.z) { r -= q.z; ++b; }
        }
    }
    bin = (uint32_t)__shfl((int)b, src, 64);
    rank = (uint32_t)__shfl((int)r, src, 64);
}

// The select of one wave over pv[0, nw): four passes, each a histogram of one byte of the values that still match the
// prefix, the scan for the bin of the rank, prefix and rank narrowed.  The first pass counts m.  REG: nw <= 64 MED_REG
// and the entries stay in registers; else every pass reads them again.  The workgroup is this one wave.
template <bool REG>
__device__ __forceinline__ void wave_select(const uint32_t *pv, uint32_t nw, uint32_t *h, int lane, uint32_t &m,
                                            uint32_t &median) {
    uint32_t v[MED_REG];
    if constexpr (REG) {
#pragma unroll
        for (int i = 0; i < MED_REG; ++i) {
            const uint32_t idx = (uint32_t)i * 64 + lane;
            v[i] = idx < nw ? pv[idx] : NO_KMER;
        }
    }
    uint32_t rank = 0, prefix = 0, himask = 0;
    m = 0; median = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        reinterpret_cast<uint4 *>(h)[lane] = make_uint4(0, 0, 0, 0);
        __syncthreads();
        if constexpr (REG) {
#pragma unroll
            for (int i = 0; i < MED_REG; ++i)
                hist_add(h, v[i] != NO_KMER && (v[i] & himask) == prefix, (v[i] >> shift) & 0xFFu, lane);
        } else {
            for (uint32_t b = 0; b < nw; b += 64) {   // (b <= nw - 1 < 2^32 - 64: a sequence line is shorter than 4 GiB - 64)
                const uint32_t idx = b + lane;
                const uint32_t x = idx < nw ? pv[idx] : NO_KMER;
                hist_add(h, x != NO_KMER && (x & himask) == prefix, (x >> shift) & 0xFFu, lane);
            }
        }
        __syncthreads();
        uint32_t bin, total;
        scan_bins(h, lane, shift == 24, rank, bin, total);
        __syncthreads();
        if (shift == 24) {
            m = total;
            if (m == 0) return;
        }
        prefix |= bin << shift;
        himask |= 0xFFu << shift;
    }
    median = prefix;
}

// med[r] = {m, median} of record rec0 <= r < min(cap, *d_nrec or nrec): its values are the entries of profile[s, e - k + 1) that
// are not NO_KMER, (s, e) its sequence line in lo (trim_lines_kernel; positions of the profile).  One wave -- one
// workgroup of 64 lanes -- per record.  A record whose sequence line is longer than long_len is not selected here: its
// index goes to list[1 + atomicAdd(list, 1)] for median_select_long_kernel (list_cap entries; a text of n bytes holds
// fewer than n / long_len such lines).  Reads of the profile stay inside [s, e - k + 1).
__global__ __launch_bounds__(64) void median_select_kernel(const uint32_t *profile, const unsigned long long *lo,
                                                           const unsigned long long *d_nrec, uint64_t rec0, uint64_t nrec,
                                                           uint64_t cap, uint32_t k, uint64_t long_len, unsigned long long *list,
                                                           uint64_t list_cap, unsigned long long *med) {
    __shared__ __attribute__((aligned(16))) uint32_t s_h[256];
    const int lane = threadIdx.x;
    const uint64_t R = min(cap, d_nrec ? (uint64_t)*d_nrec : nrec);
    for (uint64_t r = rec0 + blockIdx.x; r < R; r += gridDim.x) {
        const uint64_t s = lo[r * TL_N + 2], e = lo[r * TL_N + 3];
        uint32_t m = 0, median = 0;
        if (e >= s + k) {
            if (e - s > long_len) {
                if (lane == 0) {
                    const unsigned long long at = atomicAdd(list, 1ULL);
                    if (at < list_cap) list[1 + at] = r;
                }
                continue;
            }
            const uint32_t nw = (uint32_t)(e - s - k + 1);
            if (nw <= 64 * MED_REG) wave_select<true>(profile + s, nw, s_h, lane, m, median);
            else wave_select<false>(profile + s, nw, s_h, lane, m, median);
        }
        if (lane == 0) { med[r * 2] = m; med[r * 2 + 1] = median; }
    }
}

// The records of the list, one workgroup each.  Per pass every wave fills its own histogram from the record's entries
// -- the 16-byte aligned middle of profile[s, s + nw) as uint4, up to three entries at either end singly -- then bin b
// of the four is summed by thread b, and every wave scans the sum.
__global__ __launch_bounds__(NT) void median_select_long_kernel(const uint32_t *profile, const unsigned long long *lo,
                                                                const unsigned long long *list, uint64_t list_cap,
                                                                uint32_t k, unsigned long long *med) {
    __shared__ __attribute__((aligned(16))) uint32_t s_h[NT / 64][256];
    const int tid = threadIdx.x, lane = tid & 63;
    uint32_t *const h = s_h[tid >> 6];
    const uint64_t nl = min((uint64_t)list[0], list_cap);
    for (uint64_t li = blockIdx.x; li < nl; li += gridDim.x) {
        const uint64_t r = list[1 + li];
        const uint64_t s = lo[r * TL_N + 2], e = lo[r * TL_N + 3];
        const uint64_t nw = e - s - k + 1;   // (>= 1: the wave form lists records with e >= s + k only)
        const uint32_t *pv = profile + s;
        const uint64_t head = min(nw, (uint64_t)((4 - (s & 3)) & 3)), body = (nw - head) / 4, tail = nw - head - body * 4;
        const uint4 *pb = reinterpret_cast<const uint4 *>(pv + head);
        uint32_t rank = 0, prefix = 0, himask = 0, m = 0;
        for (int shift = 24; shift >= 0; shift -= 8) {
            __syncthreads();   // the scan of the pass (or record) before is done
            reinterpret_cast<uint4 *>(&s_h[0][0])[tid] = make_uint4(0, 0, 0, 0);
            __syncthreads();
            {
                uint32_t x = NO_KMER;
                if ((uint64_t)tid < head) x = pv[tid];
                else if ((uint64_t)tid - head < tail) x = pv[head + body * 4 + ((uint64_t)tid - head)];
                hist_add(h, x != NO_KMER && (x & himask) == prefix, (x >> shift) & 0xFFu, lane);
            }
            for (uint64_t b = 0; b < body; b += NT) {
                const uint64_t i = b + tid;
                const uint4 q = i < body ? pb[i] : make_uint4(NO_KMER, NO_KMER, NO_KMER, NO_KMER);
                hist_add(h, q.x != NO_KMER && (q.x & himask) == prefix, (q.x >> shift) & 0xFFu, lane);
                hist_add(h, q.y != NO_KMER && (q.y & himask) == prefix, (q.y >> shift) & 0xFFu, lane);
                hist_add(h, q.z != NO_KMER && (q.z & himask) == prefix, (q.z >> shift) & 0xFFu, lane);
                hist_add(h, q.w != NO_KMER && (q.w & himask) == prefix, (q.w >> shift) & 0xFFu, lane);
            }
            __syncthreads();
            {
                uint32_t t = 0;
#pragma unroll
                for (int w = 0; w < NT / 64; ++w) t += s_h[w][tid];
                s_h[0][tid] = t;   // (bin `tid` is read and written by this thread alone)
            }
            __syncthreads();
            uint32_t bin, total;
            scan_bins(s_h[0], lane, shift == 24, rank, bin, total);
            if (shift == 24) {
                m = total;
                if (m == 0) break;   // (the same in every wave)
            }
            prefix |= bin << shift;
            himask |= 0xFFu << shift;
        }
        if (tid == 0) { med[r * 2] = m; med[r * 2 + 1] = m ? prefix : 0u; }
    }
}

// The rule of tsx_hip_filter_median_host: pass iff lower <= median <= upper (a record without k-mers has median 0);
// invert writes the failures.  len and *kept as filter_len_kernel leaves them.
__global__ __launch_bounds__(NT) void median_len_kernel(const unsigned long long *med, const unsigned long long *span,
                                                        uint64_t nrec, uint64_t lower, uint64_t upper, int invert, int nl_last,
                                                        unsigned long long *len, unsigned long long *kept) {
    for (uint64_t r = (uint64_t)blockIdx.x * NT + threadIdx.x; r < nrec; r += (uint64_t)gridDim.x * NT) {
        const uint64_t md = med[r * 2 + 1];
        const bool pass = md >= lower && md <= upper;
        uint64_t l = 0;
        if (pass != (invert != 0)) l = span[r * 2 + 1] - span[r * 2] + ((nl_last && r + 1 == nrec) ? 1 : 0);
        len[r] = l;
        if (l) atomicAdd(kept, 1ULL);
    }
}

}  // namespace tsx
