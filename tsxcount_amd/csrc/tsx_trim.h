// tsx_trim.h -- abundance trimming of reads (gfx950, wave64): the solid stretch of every record, and the records cut to it.
//
//   solid_bits_kernel     the tile front end (tsx_kernels.h) and the lookup schedule (tsx_query.h); one bit per start
//                         position: "a k-mer under the base rule whose count lies in [lower, upper]" (one ballot per wave)
//   trim_lines_kernel     start and end of lines 1-4 of every record (pieces and windows of a device text)
//   trim_run_kernel       one lane per bitmap word: every run of set bits that ends in the word, walked back to its start,
//                         goes to its record with one 64-bit atomicMax of length << 32 | ~start
//   trim_finalize_kernel  unpacks that word to (start, length)
//   trim_len_kernel       the same, then the four output segments of the record (source, length) and the totals
//   trim_copy_kernel      filter_copy_kernel over segments: 16 output bytes per lane
// The segment offsets come from the u64 scan kernels of tsx_query.h.
//
// Line offsets: TL_N uint64 per record {start, end} x lines 1..4, positions in the text, end = the line's '\n' (the
// text's end for an unterminated line); an absent line is (0, 0).
#pragma once
#include "tsx_query.h"

namespace tsx {

enum { TL_N = 8 };

// Front end and lookup schedule as query_reads_kernel; then bits[w] = ballot(valid and lower <= c <= upper) for the 64
// start positions [64 w, 64 w + 64) of the text -- `bits` is the word of position 0 of buf.  Words that start at or past own_end belong to
// the next window and are not written (own_end is a multiple of 64 unless it is the text's end).
template <int WK, bool CANON = false, bool BR = false>
__global__ __launch_bounds__(NT, 2) void solid_bits_kernel(TableParams p, const uint8_t *buf, uint64_t n, uint64_t own_end,
                                                           int head_open, const uint32_t *tile_line, uint64_t ntiles,
                                                           const unsigned long long *line_base, uint64_t lower, uint64_t upper,
                                                           unsigned long long *bits, const uint16_t *qmap = nullptr) {
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
                unsigned long long word = 0;
                if (probe_round_count<WK>(p, pr, j, lane, c) != 0ULL) word = __ballot(valid && c >= lower && c <= upper);
                // the wave's 64 positions are one word: NT and BATCH are multiples of 64
                const uint64_t g0 = base + (uint64_t)(round * BATCH + j * NT + tid - lane);
                if (lane == 0 && g0 < own_end) bits[g0 >> 6] = word;
            }
        }
    }
}

// Line offsets of the records of buf[0, own_end) -- a host piece (head_open = 0, *line_base = 0, goff = 0) or a window
// of a device text at byte goff of it, whose line index continues from *line_base -- after the line pass (tile_line,
// *carry = line ends in [0, own_end)).  Line e of the text is line e & (lpr - 1) of record e >> lshift; records < cap only.
// Every start and every end is written once, by the lane that holds the byte; the end of an unterminated last line (last:
// buf + n is the text's end) by one lane of the last window.
__global__ __launch_bounds__(NT) void trim_lines_kernel(const uint8_t *buf, uint64_t n, uint64_t own_end, int head_open,
                                                        const uint32_t *tile_line, uint64_t ntiles,
                                                        const unsigned long long *line_base, const uint32_t *carry,
                                                        uint32_t lshift, uint64_t goff, int last, unsigned long long *lo,
                                                        uint64_t cap) {
    __shared__ uint32_t s_w[NT / 64];
    const int lane = threadIdx.x & 63;
    const uint64_t lbase = *line_base, lmask = (1u << lshift) - 1u;
    if (blockIdx.x == 0 && threadIdx.x == 0 && last && n > 0 && buf[n - 1] != (uint8_t)'\n') {
        const uint64_t e = lbase + *carry;
        if ((e >> lshift) < cap) lo[(e >> lshift) * TL_N + (e & lmask) * 2 + 1] = goff + n;
    }
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t off = tile * TILE + (uint64_t)threadIdx.x * 16;
        const bool pnl = prev_is_nl(buf, off, n, head_open);
        uint32_t nl, le, code;
        classify16(load16(buf, off, n), pnl, nl, le, code);
        uint32_t ls = ~nl & ((nl << 1) | (pnl ? 1u : 0u)) & 0xFFFFu;
        if (off + 16 > own_end) {   // what lies at or past own_end belongs to the next window
            const uint32_t own = (off >= own_end) ? 0u : ((1u << (own_end - off)) - 1u);
            le &= own; ls &= own;
        }
        const uint32_t c = __popc(le);
        const uint32_t inc = wave_incl_scan(c);
        if (lane == 63) s_w[threadIdx.x >> 6] = inc;
        __syncthreads();
        uint32_t woff = tile_line[tile];
        for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) woff += s_w[w];
        woff += inc - c;   // line ends before this lane's 16 bytes
        for (uint32_t b = le; b; b &= b - 1) {
            const uint32_t i = __builtin_ctz(b);
            const uint64_t e = lbase + woff + __popc(le & ((1u << i) - 1u));   // the line this '\n' ends
            if ((e >> lshift) < cap) lo[(e >> lshift) * TL_N + (e & lmask) * 2 + 1] = goff + off + i;
        }
        for (uint32_t b = ls; b; b &= b - 1) {
            const uint32_t i = __builtin_ctz(b);
            const uint64_t s = lbase + woff + __popc(le & ((1u << i) - 1u));   // line ends before the start = its index
            if ((s >> lshift) < cap) lo[(s >> lshift) * TL_N + (s & lmask) * 2] = goff + off + i;
        }
        __syncthreads();
    }
}

// span[2 r] (zeroed before) = max over the runs of record r of length << 32 | (0xFFFFFFFF - start), start counted from
// the sequence line's first byte, length in bases (windows + k - 1): the longest run, the leftmost among equals.  Both
// halves fit: a sequence line is shorter than 4 GiB.  mode 1 (prefix): only the run that starts the line.
// A run never crosses a record (the last k - 1 positions of a sequence line and its '\n' are no windows), so the run that
// ends in a word belongs to the record of its start: the last record whose first line starts at or before it, found by
// binary search over the R = min(cap, records) records that have line offsets -- a run of a later record fails the test
// against the sequence line and is dropped.  A run that reaches bit 0 walks back over the words before it.
__global__ __launch_bounds__(NT) void trim_run_kernel(const unsigned long long *bits, uint64_t nwords,
                                                      const unsigned long long *lo, const unsigned long long *d_nrec,
                                                      uint64_t nrec, uint64_t cap, uint32_t k, int mode,
                                                      unsigned long long *span) {
    const uint64_t R = min(cap, d_nrec ? (uint64_t)*d_nrec : nrec);
    if (R == 0) return;
    for (uint64_t w = (uint64_t)blockIdx.x * NT + threadIdx.x; w < nwords; w += (uint64_t)gridDim.x * NT) {
        const unsigned long long b = bits[w];
        if (b == 0) continue;
        const unsigned long long nx = (w + 1 < nwords) ? (bits[w + 1] & 1ULL) : 0ULL;
        for (unsigned long long ends = b & ~((b >> 1) | (nx << 63)); ends; ends &= ends - 1) {
            const uint32_t e = (uint32_t)__builtin_ctzll(ends);
            const unsigned long long gaps = e ? (~b & ((1ULL << e) - 1ULL)) : 0ULL;   // clear bits below the run's end
            uint64_t S;
            if (gaps) {
                S = w * 64 + (64 - (uint32_t)__builtin_clzll(gaps));
            } else {
                uint64_t ww = w;
                while (ww > 0 && bits[ww - 1] == ~0ULL) --ww;
                S = ww * 64;
                if (ww > 0) {
                    const unsigned long long z = ~bits[ww - 1];   // (not 0)
                    S -= (uint32_t)__builtin_clzll(z);
                }
            }
            const uint64_t E = w * 64 + e;
            uint64_t r = 0, hi = R;   // lo[r].start <= S < lo[hi].start
            while (hi - r > 1) {
                const uint64_t mid = (r + hi) / 2;
                if (lo[mid * TL_N] <= S) r = mid; else hi = mid;
            }
            const uint64_t s2 = lo[r * TL_N + 2], e2 = lo[r * TL_N + 3];
            if (S < s2 || E + k > e2) continue;
            if (mode == TSX_HIP_TRIM_PREFIX && S != s2) continue;
            const uint64_t len = min(E - S + k, (uint64_t)0xFFFFFFFFULL), rel = min(S - s2, (uint64_t)0xFFFFFFFFULL);
            atomicMax(span + r * 2, (unsigned long long)((len << 32) | (0xFFFFFFFFULL - rel)));
        }
    }
}

__device__ __forceinline__ void trim_unpack(unsigned long long pk, uint64_t &start, uint64_t &len) {
    len = pk >> 32;
    start = len ? 0xFFFFFFFFULL - (pk & 0xFFFFFFFFULL) : 0ULL;
}

// span[r] = (start, length) from the packed word.  Records [0, min(*nrec or nrec, cap)).
__global__ __launch_bounds__(NT) void trim_finalize_kernel(unsigned long long *span, uint64_t cap,
                                                           const unsigned long long *d_nrec, uint64_t nrec) {
    const uint64_t lim = min(cap, d_nrec ? (uint64_t)*d_nrec : nrec);
    for (uint64_t r = (uint64_t)blockIdx.x * NT + threadIdx.x; r < lim; r += (uint64_t)gridDim.x * NT) {
        uint64_t s, l;
        trim_unpack(span[r * 2], s, l);
        span[r * 2] = s; span[r * 2 + 1] = l;
    }
}

// The finalize step, then what record r contributes to the output: four segments (its lines), each src[4 r + i] = first
// text byte and seg[4 r + i] = bytes with the '\n' that follows them, 0 for an absent line or a record that is not
// written (length < min_len, min_len >= 1).  tot[0..2] += records written, bases of the sequence lines, bases kept.
__global__ __launch_bounds__(NT) void trim_len_kernel(unsigned long long *span, const unsigned long long *lo, uint64_t nrec,
                                                      uint32_t lpr, uint64_t min_len, unsigned long long *seg,
                                                      unsigned long long *src, unsigned long long *tot) {
    const uint64_t nr = (nrec + 63) & ~63ULL;   // whole waves: the totals are reduced by shuffles
    for (uint64_t r = (uint64_t)blockIdx.x * NT + threadIdx.x; r < nr; r += (uint64_t)gridDim.x * NT) {
        unsigned long long kept = 0, bin = 0, bkept = 0;
        if (r < nrec) {
            uint64_t s, l;
            trim_unpack(span[r * 2], s, l);
            span[r * 2] = s; span[r * 2 + 1] = l;
            const unsigned long long *q = lo + r * TL_N;
            const bool wr = l > 0 && l >= min_len;
            bin = q[3] - q[2];
            if (wr) { kept = 1; bkept = l; }
            const bool has3 = lpr == 4 && q[5] > q[4], has4 = lpr == 4 && q[7] > q[6];
            const uint64_t lq = q[7] - q[6], qs = min(s, lq), qe = min(s + l, lq);
            seg[r * 4 + 0] = (wr && q[1] > q[0]) ? q[1] - q[0] + 1 : 0;
            seg[r * 4 + 1] = wr ? l + 1 : 0;
            seg[r * 4 + 2] = (wr && has3) ? q[5] - q[4] + 1 : 0;
            seg[r * 4 + 3] = (wr && has4) ? qe - qs + 1 : 0;
            src[r * 4 + 0] = q[0];
            src[r * 4 + 1] = q[2] + s;
            src[r * 4 + 2] = q[4];
            src[r * 4 + 3] = q[6] + qs;
        }
        for (int d = 32; d > 0; d >>= 1) {
            kept += __shfl_down(kept, d, 64); bin += __shfl_down(bin, d, 64); bkept += __shfl_down(bkept, d, 64);
        }
        if ((threadIdx.x & 63) == 0) {
            if (kept) atomicAdd(tot + 0, kept);
            if (bin) atomicAdd(tot + 1, bin);
            if (bkept) atomicAdd(tot + 2, bkept);
        }
    }
}

// filter_copy_kernel with segments for records.  soff = exclusive scan of the segment lengths (nseg + 1 entries,
// soff[nseg] = total); segment s is text[src[s], src[s] + its length - 1) and a '\n'.  16 output bytes per lane; a wave
// finds the segment of its first byte by binary search, its lanes walk from there.  A block inside one segment's text is
// one (or two aligned) 16-byte loads; a block that crosses segments or holds a '\n' goes byte by byte.  Bytes past the
// total are written as 0 (out has the total rounded up to 16).
// (Bounds: the output never passes out_cap, the text is never read at or past tn.)
__global__ __launch_bounds__(NT) void trim_copy_kernel(const uint8_t *text, uint64_t tn, const unsigned long long *src,
                                                       const unsigned long long *soff, uint64_t nseg, uint8_t *out,
                                                       uint64_t out_cap) {
    const uint64_t total = soff[nseg];
    const uint64_t nblk = min((total + 15) / 16, out_cap / 16);
    const int lane = threadIdx.x & 63;
    for (uint64_t wb = ((uint64_t)blockIdx.x * NT + threadIdx.x) & ~63ULL; wb < nblk; wb += (uint64_t)gridDim.x * NT) {
        const uint64_t blk = wb + lane;
        // segment of the wave's first byte: the last s with soff[s] <= o (empty segments share its offset)
        uint64_t lo = 0, hi = nseg;   // soff[lo] <= o0 < soff[hi]
        const uint64_t o0 = wb * 16;
        while (hi - lo > 1) {
            const uint64_t mid = (lo + hi) / 2;
            if (soff[mid] <= o0) lo = mid; else hi = mid;
        }
        if (blk >= nblk) continue;
        const uint64_t o = blk * 16;
        uint64_t s = lo;
        while (s + 1 < nseg && soff[s + 1] <= o) ++s;
        uint64_t so = soff[s], ss = src[s], sl = soff[s + 1] - so;   // sl: bytes of the segment, its '\n' included
        uint4 v;
        if (sl && o + 16 <= so + sl - 1 && ss + sl - 1 <= tn) {
            v = load16_any(text + ss + (o - so));
        } else {
            uint32_t w[4] = {0, 0, 0, 0};
            for (uint32_t i = 0; i < 16; ++i) {
                const uint64_t q = o + i;
                if (q >= total) break;
                while (s + 1 < nseg && soff[s + 1] <= q) {
                    ++s;
                    so = soff[s]; ss = src[s]; sl = soff[s + 1] - so;
                }
                const uint64_t a = ss + (q - so);
                const uint32_t b = (q - so + 1 < sl && a < tn) ? text[a] : (uint32_t)'\n';
                w[i >> 2] |= b << (8 * (i & 3));
            }
            v = make_uint4(w[0], w[1], w[2], w[3]);
        }
        *reinterpret_cast<uint4 *>(out + o) = v;
    }
}

}  // namespace tsx
