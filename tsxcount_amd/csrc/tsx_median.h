// tsx_median.h -- the median k-mer abundance of reads (gfx950, wave64): the count of every window of a text, the
// median of every record's counts, and the filter on it.
//
//   window_counts_kernel       solid_bits_kernel up to the shuffle that hands followers their leader's count; then one
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
template <int WK, bool CANON = false, bool BR = false>
__global__ __launch_bounds__(NT, 2) void window_counts_kernel(TableParams p, const uint8_t *buf, uint64_t n, uint64_t own_end,
                                                              int head_open, const uint32_t *tile_line, uint64_t ntiles,
                                                              const unsigned long long *line_base, uint32_t *profile,
                                                              const uint16_t *qmap = nullptr) {
    __shared__ uint64_t s_codes[(TILE + HALO) / 32 + 2];
    __shared__ uint64_t s_nl[(TILE + HALO) / 64 + 3];
    __shared__ uint64_t s_le[TILE / 64];
    __shared__ uint32_t s_lb[TILE / 16];
    __shared__ uint32_t s_wsum[NT / 64];
    extern __shared__ uint64_t s_lut[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int lut_words = p.groups * (1 << p.g) * WK;
    for (int i = tid; i < lut_words; i += NT) s_lut[i] = p.lut[i];
    if (tid < 3) s_nl[(TILE + HALO) / 64 + tid] = ~0ULL;
    if (tid < 2) s_codes[(TILE + HALO) / 32 + tid] = 0;
    const uint32_t k = (uint32_t)p.k;
    const uint64_t lbase = *line_base;
    const uint64_t need0 = (k >= 64) ? ~0ULL : ((1ULL << k) - 1ULL);
    const uint64_t need1 = (k > 64) ? ((k >= 128) ? ~0ULL : ((1ULL << (k - 64)) - 1ULL)) : 0ULL;
    const unsigned long long below = (lane == 0) ? 0ULL : (~0ULL >> (64 - lane));   // lanes < lane
    const uint64_t wr_end = min(own_end, n);
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
            uint64_t hk[PER_THREAD][WK];
            uint64_t v1[PER_THREAD];
            uint32_t vbits = 0, lbits = 0;   // bit j: position j is valid / a run leader
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
                v1[j] = 0;
                if (__ballot(valid) == 0ULL) continue;
                uint64_t x[WK];
                extract_kmer<WK>(s_codes, pp, p.top_mask, x);
                uint64_t xp[WK];
#pragma unroll
                for (int t = 0; t < WK; ++t) xp[t] = __shfl_up((unsigned long long)x[t], 1, 64);
                const bool prev_valid = __shfl_up((int)valid, 1, 64) != 0;
                const bool leader = valid && (lane == 0 || !prev_valid || !kmer_eq<WK>(x, xp));
                vbits |= valid ? (1u << j) : 0u;
                lbits |= leader ? (1u << j) : 0u;
                if (leader) {
                    hash_key<CANON, WK>(p, (const uint64_t *)s_lut, x, hk[j]);
                    v1[j] = first_probe<WK>(p, hk[j]);
                }
            }
#pragma unroll
            for (int j = 0; j < PER_THREAD; ++j) {
                const bool valid = (vbits >> j) & 1u, leader = (lbits >> j) & 1u;
                uint32_t out = NO_KMER;
                if (__ballot(valid) != 0ULL) {
                    uint64_t c = leader ? lookup_rest<WK>(p, hk[j], v1[j]) : 0;
                    // followers: the nearest leader at or below the lane holds the same k-mer
                    const unsigned long long lmask = __ballot(leader) & (below | (1ULL << lane));
                    const int src = lmask ? 63 - __builtin_clzll(lmask) : lane;
                    c = __shfl((unsigned long long)c, src, 64);
                    if (valid) out = (uint32_t)min(c, (uint64_t)(NO_KMER - 1u));
                }
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

// med[r] = {m, median} of record r < min(cap, *d_nrec or nrec): its values are the entries of profile[s, e - k + 1) that
// are not NO_KMER, (s, e) its sequence line in lo (trim_lines_kernel; positions of the profile).  One wave -- one
// workgroup of 64 lanes -- per record.  A record whose sequence line is longer than long_len is not selected here: its
// index goes to list[1 + atomicAdd(list, 1)] for median_select_long_kernel (list_cap entries; a text of n bytes holds
// fewer than n / long_len such lines).  Reads of the profile stay inside [s, e - k + 1).
__global__ __launch_bounds__(64) void median_select_kernel(const uint32_t *profile, const unsigned long long *lo,
                                                           const unsigned long long *d_nrec, uint64_t nrec, uint64_t cap,
                                                           uint32_t k, uint64_t long_len, unsigned long long *list,
                                                           uint64_t list_cap, unsigned long long *med) {
    __shared__ __attribute__((aligned(16))) uint32_t s_h[256];
    const int lane = threadIdx.x;
    const uint64_t R = min(cap, d_nrec ? (uint64_t)*d_nrec : nrec);
    for (uint64_t r = blockIdx.x; r < R; r += gridDim.x) {
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
