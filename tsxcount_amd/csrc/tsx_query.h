// tsx_query.h -- read queries against a filled table (gfx950, wave64): per-record k-mer statistics and the read filter.
//
//   query_reads_kernel     the tile front end (tsx_kernels.h) with the FULL line index and the lookup schedule below
//                          (run-length merge, hash_key, a lookup in place of the insert), then a segmented per-record
//                          reduction across the wave that ends in one set of global atomics per (wave, record) run
//   query_finalize_kernel  min_count of every record: the kernel keeps ~min under atomicMax; 0 for records without k-mers
//   query_window_kernel    device texts in windows: the line base of the next window, the record count after the last
//   record_scan_kernel     host pieces: where the last whole record of a piece ends, how many records it holds, and the
//                          byte span [start, end) of each of them (the filter copies spans)
//   filter_len_kernel      the pass / fail rule per record -> bytes it contributes to the output
//   u64 scan kernels       exclusive scan of those lengths
//   filter_copy_kernel     output-driven compaction: 16 output bytes per lane, 16-byte loads where the source allows
//
// Stats layout: four uint64 per record {kmers, in_range, min_count, sum_count} (tsx_hip_read_stats).
#pragma once
#include "tsx_kernels.h"

namespace tsx {

enum { QS_KMERS = 0, QS_INRANGE = 1, QS_MIN = 2, QS_SUM = 3, QS_N = 4 };

// getKmerCount (TSXHashMap.h:548-638) in two halves, so that a lane can issue the first probe load of all its
// positions before it waits for any of them (the loads are random HBM reads: latency, not bandwidth, bounds them).
// The map is not a shard (the entry points refuse shard maps): no owner test here.
template <int WK>
__device__ __forceinline__ uint64_t first_probe(const TableParams &p, const uint64_t (&h)[WK]) {
    const uint64_t pos0 = h[0] & p.slot_mask;
    return p.table[probe_pos(p, pos0, 1) * (uint64_t)p.W];
}
template <int WK>
__device__ inline uint64_t lookup_rest(const TableParams &p, const uint64_t (&h)[WK], uint64_t v) {
    uint64_t pos0, e0, hi[4];
    split_key<WK>(p, h, pos0, e0, hi);
    const int W = p.W;
    for (uint32_t i = 1; i <= p.max_reprobes; ++i) {
        const uint64_t pos = probe_pos(p, pos0, i);
        const uint64_t *e = p.table + pos * (uint64_t)W;
        if (i > 1) v = e[0];
        if (v == 0) return 0;
        if ((v & p.k0mask) != (e0 | i)) continue;
        bool same = true;
        for (int t = 1; t < W; ++t) same &= (e[t] == hi[t - 1]);
        if (!same) continue;
        return (v >> p.cshift) + (sec_get(p, pos) << p.C);
    }
    return 0;
}

// The lookup schedule of a round of BATCH start positions (query_reads_kernel, solid_bits_kernel, window_counts_kernel).
// probe_round_issue: for every position of the lane the window test, extraction and the run-leader test; leaders hash
// and issue their first probe load -- all PER_THREAD loads before any is waited for.  It leaves bit j of vbits / lbits
// (position j is valid / a run leader) and, for leaders, hk[j] and v1[j].
template <int WK>
struct ProbeRound {
    uint64_t hk[PER_THREAD][WK];
    uint64_t v1[PER_THREAD];
    uint32_t vbits, lbits;
};
template <bool CANON, int WK>
__device__ __forceinline__ void probe_round_issue(const TableParams &p, const uint64_t *lut, const TileLds<uint32_t> &s,
                                                  const WindowRule &rule, uint64_t base, int round, int tid,
                                                  ProbeRound<WK> &pr) {
    pr.vbits = 0; pr.lbits = 0;
#pragma unroll
    for (int j = 0; j < PER_THREAD; ++j) {
        const uint32_t pp = (uint32_t)(round * BATCH + j * NT + tid);
        uint32_t line;
        const bool valid = window_valid(s, rule, base, pp, line);
        pr.v1[j] = 0;
        if (__ballot(valid) == 0ULL) continue;
        uint64_t x[WK];
        extract_kmer<WK>(s.codes, pp, p.top_mask, x);
        const bool leader = run_leader<WK>(x, valid, tid & 63);
        pr.vbits |= valid ? (1u << j) : 0u;
        pr.lbits |= leader ? (1u << j) : 0u;
        if (leader) {
            hash_key<CANON, WK>(p, lut, x, pr.hk[j]);
            pr.v1[j] = first_probe<WK>(p, pr.hk[j]);
        }
    }
}
// probe_round_count: position j of the round.  Returns the ballot of the valid lanes; when it is not empty, c is the
// count of the lane's k-mer for every valid lane: leaders finish their probe, followers (equal k-mer in the lane below)
// take the count of the nearest leader at or below them by shuffle.  Called by whole waves.
template <int WK>
__device__ __forceinline__ unsigned long long probe_round_count(const TableParams &p, const ProbeRound<WK> &pr, int j,
                                                                int lane, uint64_t &c) {
    const bool valid = (pr.vbits >> j) & 1u, leader = (pr.lbits >> j) & 1u;
    const unsigned long long vmask = __ballot(valid);
    c = 0;
    if (vmask == 0ULL) return vmask;
    if (leader) c = lookup_rest<WK>(p, pr.hk[j], pr.v1[j]);
    const unsigned long long lmask = __ballot(leader) & (~0ULL >> (63 - lane));   // leaders at or below the lane
    const int src = lmask ? 63 - __builtin_clzll(lmask) : lane;
    c = __shfl((unsigned long long)c, src, 64);
    return vmask;
}

// Per tile the front end (tile_load, tile_stage).  The line index is kept whole
// (32 bits: one window holds fewer than 2^32 lines) and offset by *line_base (lines of the earlier windows), so that
// the record of a window is (line_base + line) >> lshift.  Then per round of BATCH start positions:
//   A. probe_round_issue;
//   B. per position probe_round_count; the
//      valid lanes of a wave form runs, one run per record (positions of one record are contiguous, those of two
//      records are separated by invalid positions); a segmented suffix reduction leaves the run's kmers, in_range,
//      sum and min at its first lane, which adds them to the record with four global atomics.
// stats[r] is written for r < cap only.
// BR (base rule): windows the rule drops are not k-mers of the read (rule_bits16, as the count kernels).
template <int WK, bool CANON = false, bool BR = false>
__global__ __launch_bounds__(NT, 2) void query_reads_kernel(TableParams p, const uint8_t *buf, uint64_t n, uint64_t own_end,
                                                            int head_open, const uint32_t *tile_line, uint64_t ntiles,
                                                            const unsigned long long *line_base, uint32_t lshift,
                                                            uint64_t lower, uint64_t upper, unsigned long long *stats,
                                                            uint64_t cap, const uint16_t *qmap = nullptr) {
    __shared__ TileLds<uint32_t> s;
    extern __shared__ uint64_t s_lut[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int lut_words = p.groups * (1 << p.g) * WK;
    for (int i = tid; i < lut_words; i += NT) s_lut[i] = p.lut[i];
    s.set_sentinels(tid);
    const WindowRule rule(p, n, own_end, *line_base);
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
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
                const unsigned long long vmask = probe_round_count<WK>(p, pr, j, lane, c);
                if (vmask == 0ULL) continue;
                // runs of valid lanes: head = first lane of a run; seg = lanes from this one to the end of its run
                const bool head = valid && (lane == 0 || !((vmask >> (lane - 1)) & 1ULL));
                const uint32_t seg = run_length(head, valid, lane);
                unsigned long long sum = valid ? c : 0ULL, mn = valid ? c : ~0ULL;
                uint32_t inr = (valid && c >= lower && c <= upper) ? 1u : 0u;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const unsigned long long os = __shfl_down(sum, d, 64), om = __shfl_down(mn, d, 64);
                    const uint32_t oi = __shfl_down(inr, d, 64);
                    if ((uint32_t)d < seg) { sum += os; mn = om < mn ? om : mn; inr += oi; }
                }
                if (head) {
                    const uint32_t line = tile_line_of(s, (uint32_t)(round * BATCH + j * NT + tid));
                    const uint64_t rec = (rule.lbase + line) >> lshift;
                    if (rec < cap) {
                        unsigned long long *st = stats + rec * QS_N;
                        atomicAdd(st + QS_KMERS, (unsigned long long)seg);
                        if (inr) atomicAdd(st + QS_INRANGE, (unsigned long long)inr);
                        atomicAdd(st + QS_SUM, sum);
                        atomicMax(st + QS_MIN, ~mn);
                    }
                }
            }
        }
    }
}

// min_count = ~(the atomicMax of ~c), 0 for records without k-mers.  Records [0, min(*nrec or nrec, cap)).
__global__ __launch_bounds__(NT) void query_finalize_kernel(unsigned long long *stats, uint64_t cap,
                                                            const unsigned long long *d_nrec, uint64_t nrec) {
    const uint64_t lim = min(cap, d_nrec ? (uint64_t)*d_nrec : nrec);
    for (uint64_t r = (uint64_t)blockIdx.x * NT + threadIdx.x; r < lim; r += (uint64_t)gridDim.x * NT) {
        unsigned long long *s = stats + r * QS_N;
        s[QS_MIN] = s[QS_KMERS] ? ~s[QS_MIN] : 0ULL;
    }
}

// One lane, after the query kernel of a window: line_base += the window's line ends (*carry).  After the last window
// (last = 1): *nrec = ceil(lines / lines_per_record), lines counting an unterminated last line (buf_last: the text's
// last byte, NULL for an empty text).
__global__ void query_window_kernel(unsigned long long *line_base, const uint32_t *carry, int last, const uint8_t *buf_last,
                                    uint32_t lpr, unsigned long long *nrec) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    unsigned long long lines = *line_base + *carry;
    *line_base = lines;
    if (last) {
        if (buf_last && *buf_last != (uint8_t)'\n') ++lines;
        *nrec = (lines + lpr - 1) / lpr;
    }
}

// A host piece [0, n) that starts at a record boundary, after the line pass (tile_line, *carry = line ends).
//   info[0] = cut: the end of the last whole record (last piece: n), info[1] = records in [0, cut), info[2] = 1 when the
//   last record's last line has no '\n' (last piece only).  Not last and no whole record: info[1] = 0.
//   span (2 words per record, optional, records < span_cap): first byte of its first line, end of its last line
//   (past its '\n'; the text's end for an unterminated line).
// Line starts and ends come from the same classify16 masks as the scan kernels.
__global__ __launch_bounds__(NT) void record_scan_kernel(const uint8_t *buf, uint64_t n, const uint32_t *tile_line,
                                                         uint64_t ntiles, const uint32_t *carry, uint32_t lpr, int last,
                                                         unsigned long long *info, unsigned long long *span,
                                                         uint64_t span_cap) {
    __shared__ uint32_t s_w[NT / 64];
    const int lane = threadIdx.x & 63;
    const uint64_t L = *carry;                                          // line ends in the piece
    const bool open = last && n > 0 && buf[n - 1] != (uint8_t)'\n';     // unterminated last line
    const uint64_t lines = L + (open ? 1 : 0);
    const uint64_t R = last ? (lines + lpr - 1) / lpr : L / lpr;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        info[1] = R;
        info[2] = open ? 1 : 0;
        if (last) info[0] = n;
        else if (R == 0) info[0] = 0;
        if (span && open && R - 1 < span_cap) span[(R - 1) * 2 + 1] = n;
    }
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t off = tile * TILE + (uint64_t)threadIdx.x * 16;
        const bool pnl = prev_is_nl(buf, off, n, 0);
        uint32_t nl, le, code;
        classify16(load16(buf, off, n), pnl, nl, le, code);
        if (off + 16 > n) le &= (off >= n) ? 0u : ((1u << (n - off)) - 1u);
        const uint32_t prev = (nl << 1) | (pnl ? 1u : 0u);
        uint32_t ls = ~nl & prev & 0xFFFFu;
        if (off + 16 > n) ls &= (off >= n) ? 0u : ((1u << (n - off)) - 1u);
        const uint32_t c = __popc(le);
        const uint32_t inc = wave_incl_scan(c);
        if (lane == 63) s_w[threadIdx.x >> 6] = inc;
        __syncthreads();
        uint32_t woff = tile_line[tile];
        for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) woff += s_w[w];
        woff += inc - c;   // line ends before this lane's 16 bytes
        for (uint32_t b = le; b; b &= b - 1) {
            const uint32_t i = __builtin_ctz(b);
            const uint64_t e = woff + __popc(le & ((1u << i) - 1u));   // index of the line this '\n' ends
            const uint64_t r = e / lpr;
            const bool closes = (e % lpr == lpr - 1) || (last && !open && e + 1 == L);
            if (closes && r < R) {
                if (span && r < span_cap) span[r * 2 + 1] = off + i + 1;
                if (!last && r + 1 == R) info[0] = off + i + 1;
            }
        }
        for (uint32_t b = ls; b; b &= b - 1) {
            const uint32_t i = __builtin_ctz(b);
            const uint64_t s = woff + __popc(le & ((1u << i) - 1u));   // line ends before the start = its line index
            if (s % lpr == 0 && s / lpr < R && span && s / lpr < span_cap) span[(s / lpr) * 2] = off + i;
        }
        __syncthreads();
    }
}

// The filter's rule for one record: in_range >= min_in_range and in_range * 10^6 >= ppm * kmers (exact, 128-bit products).
__device__ __forceinline__ bool filter_pass(uint64_t km, uint64_t inr, uint64_t min_in, uint64_t ppm) {
    const uint64_t ah = __umul64hi(inr, 1000000ULL), al = inr * 1000000ULL;
    const uint64_t bh = __umul64hi(ppm, km), bl = ppm * km;
    return (inr >= min_in) && (ah > bh || (ah == bh && al >= bl));
}

// The rule of tsx_hip_filter_reads_host: pass iff in_range >= min_in_range and in_range * 10^6 >= ppm * kmers (exact,
// 128-bit products); invert writes the failures.  len[r] = bytes record r contributes: its span, plus the '\n' the text
// lacks for the last record when nl_last; *kept counts the records written.
__global__ __launch_bounds__(NT) void filter_len_kernel(const unsigned long long *stats, const unsigned long long *span,
                                                        uint64_t nrec, uint64_t min_in, uint64_t ppm, int invert, int nl_last,
                                                        unsigned long long *len, unsigned long long *kept) {
    for (uint64_t r = (uint64_t)blockIdx.x * NT + threadIdx.x; r < nrec; r += (uint64_t)gridDim.x * NT) {
        const bool pass = filter_pass(stats[r * QS_N + QS_KMERS], stats[r * QS_N + QS_INRANGE], min_in, ppm);
        uint64_t l = 0;
        if (pass != (invert != 0)) l = span[r * 2 + 1] - span[r * 2] + ((nl_last && r + 1 == nrec) ? 1 : 0);
        len[r] = l;
        if (l) atomicAdd(kept, 1ULL);
    }
}

// Exclusive scan of n uint64 in place, three launches as the line scan: chunk sums, one workgroup over the chunk sums
// (leaving the total in *total), the scan inside each chunk.
__global__ __launch_bounds__(SCAN_CHUNK) void u64_chunk_sum_kernel(const unsigned long long *v, uint64_t n,
                                                                  unsigned long long *chunk_sum) {
    __shared__ unsigned long long s_w[SCAN_CHUNK / 64];
    const uint64_t i = (uint64_t)blockIdx.x * SCAN_CHUNK + threadIdx.x;
    unsigned long long x = (i < n) ? v[i] : 0;
    for (int d = 32; d > 0; d >>= 1) x += __shfl_down(x, d, 64);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = x;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (int w = 0; w < SCAN_CHUNK / 64; ++w) t += s_w[w];
        chunk_sum[blockIdx.x] = t;
    }
}
__global__ __launch_bounds__(1024) void u64_chunk_scan_kernel(unsigned long long *chunk_sum, uint64_t nchunks,
                                                              unsigned long long *total) {
    __shared__ unsigned long long s_w[16];
    __shared__ unsigned long long s_base;
    if (threadIdx.x == 0) s_base = 0;
    __syncthreads();
    for (uint64_t start = 0; start < nchunks; start += 1024) {
        const uint64_t i = start + threadIdx.x;
        const unsigned long long x = (i < nchunks) ? chunk_sum[i] : 0;
        const unsigned long long inc = wave_incl_scan64(x);
        if ((threadIdx.x & 63) == 63) s_w[threadIdx.x >> 6] = inc;
        __syncthreads();
        unsigned long long woff = 0;
        for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) woff += s_w[w];
        const unsigned long long b = s_base;
        if (i < nchunks) chunk_sum[i] = b + woff + inc - x;
        __syncthreads();
        if (threadIdx.x == 1023) s_base = b + woff + inc;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = s_base;
}
__global__ __launch_bounds__(SCAN_CHUNK) void u64_scan_kernel(unsigned long long *v, uint64_t n,
                                                             const unsigned long long *chunk_base) {
    __shared__ unsigned long long s_w[SCAN_CHUNK / 64];
    const uint64_t i = (uint64_t)blockIdx.x * SCAN_CHUNK + threadIdx.x;
    const unsigned long long x = (i < n) ? v[i] : 0;
    const unsigned long long inc = wave_incl_scan64(x);
    if ((threadIdx.x & 63) == 63) s_w[threadIdx.x >> 6] = inc;
    __syncthreads();
    unsigned long long woff = chunk_base[blockIdx.x];
    for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) woff += s_w[w];
    if (i < n) v[i] = woff + inc - x;
}

// 16 bytes from any address p of a buffer that is readable up to the next 16-byte boundary past p + 15: two aligned
// 16-byte loads and a funnel shift (one load when p is aligned).
__device__ __forceinline__ uint4 load16_any(const uint8_t *p) {
    const uintptr_t a = (uintptr_t)p;
    const uint4 *q = reinterpret_cast<const uint4 *>(a & ~(uintptr_t)15);
    const uint32_t sh = (uint32_t)(a & 15);
    const uint4 x = q[0];
    if (sh == 0) return x;
    const uint4 y = q[1];
    uint64_t w0 = ((uint64_t)x.y << 32) | x.x, w1 = ((uint64_t)x.w << 32) | x.z;
    uint64_t w2 = ((uint64_t)y.y << 32) | y.x, w3 = ((uint64_t)y.w << 32) | y.z;
    uint32_t s = sh * 8;
    if (s >= 64) { w0 = w1; w1 = w2; w2 = w3; s -= 64; }
    const uint64_t lo = s ? ((w0 >> s) | (w1 << (64 - s))) : w0;
    const uint64_t hi = s ? ((w1 >> s) | (w2 << (64 - s))) : w1;
    return make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
}

// The output, 16 bytes per lane: out[o .. o+16) for o = 16 * lane index.  koff = exclusive scan of the kept lengths
// (nrec + 1 entries, koff[nrec] = total).  A wave finds the record of its first byte by binary search, its lanes walk
// from there.  A block inside one record's text is one (or two aligned) 16-byte loads; a block that crosses records or
// holds the appended '\n' goes byte by byte.  Bytes past the total are written as 0 (out has the total rounded up to 16).
// (Bounds: the output never passes out_cap, the text is never read at or past tn.)
__global__ __launch_bounds__(NT) void filter_copy_kernel(const uint8_t *text, uint64_t tn, const unsigned long long *span,
                                                         const unsigned long long *koff, uint64_t nrec, uint8_t *out,
                                                         uint64_t out_cap) {
    const uint64_t total = koff[nrec];
    const uint64_t nblk = min((total + 15) / 16, out_cap / 16);
    const int lane = threadIdx.x & 63;
    for (uint64_t wb = ((uint64_t)blockIdx.x * NT + threadIdx.x) & ~63ULL; wb < nblk; wb += (uint64_t)gridDim.x * NT) {
        const uint64_t blk = wb + lane;
        // record of the wave's first byte: the last r with koff[r] <= o (records that keep nothing share its offset)
        uint64_t lo = 0, hi = nrec;   // koff[lo] <= o0 < koff[hi]
        const uint64_t o0 = wb * 16;
        while (hi - lo > 1) {
            const uint64_t mid = (lo + hi) / 2;
            if (koff[mid] <= o0) lo = mid; else hi = mid;
        }
        if (blk >= nblk) continue;
        const uint64_t o = blk * 16;
        uint64_t r = lo;
        while (r + 1 < nrec && koff[r + 1] <= o) ++r;
        const uint64_t ro = koff[r], rs = span[r * 2], rl = span[r * 2 + 1] - rs;   // rl: text bytes of the record
        uint4 v;
        if (o + 16 <= ro + rl && rs + rl <= tn) {
            v = load16_any(text + rs + (o - ro));
        } else {
            uint32_t w[4] = {0, 0, 0, 0};
            uint64_t rr = r, rro = ro, rrs = rs, rrl = rl;
            for (uint32_t i = 0; i < 16; ++i) {
                const uint64_t q = o + i;
                if (q >= total) break;
                while (rr + 1 < nrec && koff[rr + 1] <= q) {
                    ++rr;
                    rro = koff[rr]; rrs = span[rr * 2]; rrl = span[rr * 2 + 1] - rrs;
                }
                const uint32_t b = (q - rro < rrl) ? (rrs + (q - rro) < tn ? text[rrs + (q - rro)] : 0u) : (uint32_t)'\n';
                w[i >> 2] |= b << (8 * (i & 3));
            }
            v = make_uint4(w[0], w[1], w[2], w[3]);
        }
        *reinterpret_cast<uint4 *>(out + o) = v;
    }
}

}  // namespace tsx
