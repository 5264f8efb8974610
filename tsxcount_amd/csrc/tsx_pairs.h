// tsx_pairs.h -- mate pairs kept in step (gfx950, wave64): what the paired filter and the paired trim add around the
// kernels of tsx_query.h and tsx_trim.h.  Mate 1 and mate 2 of pair i are record i of two texts A and B, or records 2 i
// and 2 i + 1 of one interleaved text.
//
//   pair_cut_kernel          one lane, after the record scans of a piece of A and a piece of B: R = the records both
//                            pieces hold, and where record R - 1 of each ends (from the spans)
//   pair_names_kernel        one lane per pair: the names of the two header lines, byte for byte
//   pair_gate_filter_kernel  one lane per pair: both verdicts -> the bytes each mate gives to the kept-pair outputs and
//                            to the orphan outputs
//   pair_gate_trim_kernel    the same over the four segments per record of trim_len_kernel
// The gated lengths then go through the u64 scan kernels and filter_copy_kernel / trim_copy_kernel, one output at a time.
//
// Both forms run the same kernels: every per-record array of mate 2 is a pointer of its own, and `stride` is the distance
// between the records of consecutive pairs -- 1 with two texts; 2 with an interleaved text, where mate 2's arrays are
// mate 1's moved on by one record.
#pragma once
#include "tsx_trim.h"

namespace tsx {

// words of the pair info block (device, and its pinned copy)
enum { PI_R = 0, PI_CUT_A = 1, PI_CUT_B = 2, PI_RA = 3, PI_RB = 4, PI_OPEN_A = 5, PI_OPEN_B = 6,
       PI_KEPT = 8, PI_SINGLE_A = 9, PI_SINGLE_B = 10, PI_BAD = 11, PI_TOTAL = 12 /* 4 outputs */,
       PI_TRIM_A = 16 /* records written, bases in, bases kept */, PI_TRIM_B = 19, PI_N = 24 };

// info_a / info_b: what record_scan_kernel left for the two pieces (cut, records, open); info_b == NULL: one interleaved
// text.  pi[PI_RA], pi[PI_RB] = the records of each piece; pi[PI_R] = the records of each piece that this round takes:
// min(RA, RB), or for an interleaved piece RA without its last record when RA is odd and the piece is not the text's
// last (an odd last piece keeps RA: the host refuses it).  pi[PI_CUT_*] = where the next piece of each text starts: the
// scan's own cut when the round takes all records of the piece, else the end of record R - 1; pi[PI_OPEN_*] = the
// unterminated last line, only when the round takes the record that has it.
__global__ void pair_cut_kernel(const unsigned long long *info_a, const unsigned long long *span_a,
                                const unsigned long long *info_b, const unsigned long long *span_b, int last_a,
                                unsigned long long *pi) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const unsigned long long ra = info_a[1], rb = info_b ? info_b[1] : 0ULL;
    unsigned long long r;
    if (info_b) r = ra < rb ? ra : rb;
    else r = last_a ? ra : (ra & ~1ULL);
    pi[PI_RA] = ra; pi[PI_RB] = rb; pi[PI_R] = r;
    pi[PI_CUT_A] = (r == ra) ? info_a[0] : (r ? span_a[(r - 1) * 2 + 1] : 0ULL);
    pi[PI_OPEN_A] = (r == ra) ? info_a[2] : 0ULL;
    pi[PI_CUT_B] = !info_b ? 0ULL : (r == rb) ? info_b[0] : (r ? span_b[(r - 1) * 2 + 1] : 0ULL);
    pi[PI_OPEN_B] = (info_b && r == rb) ? info_b[2] : 0ULL;
}

// The name of the record text[s, e): the bytes after the first one up to the first space, tab or line end, without one
// trailing "/1" or "/2".  Returns its length; `from` = its first byte.
__device__ __forceinline__ uint64_t pair_name_of(const uint8_t *text, uint64_t s, uint64_t e, uint64_t &from) {
    from = s + 1;
    uint64_t p = from;
    while (p < e) {
        const uint8_t c = text[p];
        if (c == (uint8_t)' ' || c == (uint8_t)'\t' || c == (uint8_t)'\n') break;
        ++p;
    }
    uint64_t len = p > from ? p - from : 0;
    if (len >= 2 && text[from + len - 2] == (uint8_t)'/' && (text[from + len - 1] == (uint8_t)'1' || text[from + len - 1] == (uint8_t)'2'))
        len -= 2;
    return len;
}

// *bad (zeroed before) = ~(the first pair whose mates' names differ), 0 when all agree.  The spans bound every read:
// span ends never pass the piece's cut.
__global__ __launch_bounds__(NT) void pair_names_kernel(const uint8_t *text_a, const unsigned long long *span_a,
                                                        const uint8_t *text_b, const unsigned long long *span_b,
                                                        uint64_t npairs, uint32_t stride, unsigned long long *bad) {
    for (uint64_t i = (uint64_t)blockIdx.x * NT + threadIdx.x; i < npairs; i += (uint64_t)gridDim.x * NT) {
        const uint64_t r = i * stride;
        uint64_t fa, fb;
        const uint64_t la = pair_name_of(text_a, span_a[r * 2], span_a[r * 2 + 1], fa);
        const uint64_t lb = pair_name_of(text_b, span_b[r * 2], span_b[r * 2 + 1], fb);
        bool same = la == lb;
        for (uint64_t j = 0; same && j < la; ++j) same = text_a[fa + j] == text_b[fb + j];
        if (!same) atomicMax(bad, ~(unsigned long long)i);
    }
}

// tot[0..2] += a, b, c summed over the wave: one atomic per wave and counter.
__device__ __forceinline__ void pair_wave_totals(unsigned long long a, unsigned long long b, unsigned long long c,
                                                 unsigned long long *tot) {
    for (int d = 32; d > 0; d >>= 1) {
        a += __shfl_down(a, d, 64); b += __shfl_down(b, d, 64); c += __shfl_down(c, d, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (a) atomicAdd(tot + 0, a);
        if (b) atomicAdd(tot + 1, b);
        if (c) atomicAdd(tot + 2, c);
    }
}

// Pair i: the verdict of each mate is filter_len_kernel's (invert included).  any == 0: the pair is kept when both hold,
// and a mate that holds alone is an orphan; any != 0: kept when one holds, no orphans.  keep_*[r] / single_*[r] = the
// bytes record r gives to the kept-pair output / the orphan output of its side: its span, plus the '\n' the text lacks
// for the last record of the side when nl_*.  tot[0..2] += pairs kept, orphans of A, orphans of B.
__global__ __launch_bounds__(NT) void pair_gate_filter_kernel(const unsigned long long *stats_a, const unsigned long long *span_a,
                                                              const unsigned long long *stats_b, const unsigned long long *span_b,
                                                              uint64_t npairs, uint32_t stride, uint64_t min_in, uint64_t ppm,
                                                              int invert, int any, int nl_a, int nl_b,
                                                              unsigned long long *keep_a, unsigned long long *keep_b,
                                                              unsigned long long *single_a, unsigned long long *single_b,
                                                              unsigned long long *tot) {
    const uint64_t np = (npairs + 63) & ~63ULL;   // whole waves: the totals are reduced by shuffles
    for (uint64_t i = (uint64_t)blockIdx.x * NT + threadIdx.x; i < np; i += (uint64_t)gridDim.x * NT) {
        unsigned long long kept = 0, oa = 0, ob = 0;
        if (i < npairs) {
            const uint64_t r = i * stride;
            const bool va = filter_pass(stats_a[r * QS_N + QS_KMERS], stats_a[r * QS_N + QS_INRANGE], min_in, ppm) != (invert != 0);
            const bool vb = filter_pass(stats_b[r * QS_N + QS_KMERS], stats_b[r * QS_N + QS_INRANGE], min_in, ppm) != (invert != 0);
            const bool last = i + 1 == npairs;
            const uint64_t la = span_a[r * 2 + 1] - span_a[r * 2] + ((nl_a && last) ? 1 : 0);
            const uint64_t lb = span_b[r * 2 + 1] - span_b[r * 2] + ((nl_b && last) ? 1 : 0);
            const bool pair = any ? (va || vb) : (va && vb);
            kept = pair ? 1 : 0;
            oa = (!any && va && !vb) ? 1 : 0;
            ob = (!any && vb && !va) ? 1 : 0;
            keep_a[r] = pair ? la : 0; keep_b[r] = pair ? lb : 0;
            single_a[r] = oa ? la : 0; single_b[r] = ob ? lb : 0;
        }
        pair_wave_totals(kept, oa, ob, tot);
    }
}

// Pair i over the segments of trim_len_kernel (seg_*[4 r + j], before their scan): a mate survives when its sequence
// segment is written (seg[4 r + 1] != 0).  Both survive: the pair is kept, the segments of both go to keep_*; one
// survives: an orphan, its segments go to single_* of its side.  tot[0..2] += pairs kept, orphans of A, orphans of B.
__global__ __launch_bounds__(NT) void pair_gate_trim_kernel(const unsigned long long *seg_a, const unsigned long long *seg_b,
                                                            uint64_t npairs, uint32_t stride, unsigned long long *keep_a,
                                                            unsigned long long *keep_b, unsigned long long *single_a,
                                                            unsigned long long *single_b, unsigned long long *tot) {
    const uint64_t np = (npairs + 63) & ~63ULL;
    for (uint64_t i = (uint64_t)blockIdx.x * NT + threadIdx.x; i < np; i += (uint64_t)gridDim.x * NT) {
        unsigned long long kept = 0, oa = 0, ob = 0;
        if (i < npairs) {
            const uint64_t q = i * stride * 4;
            unsigned long long a[4], b[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) { a[j] = seg_a[q + j]; b[j] = seg_b[q + j]; }
            const bool sa = a[1] != 0, sb = b[1] != 0;
            kept = (sa && sb) ? 1 : 0; oa = (sa && !sb) ? 1 : 0; ob = (sb && !sa) ? 1 : 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                keep_a[q + j] = kept ? a[j] : 0; keep_b[q + j] = kept ? b[j] : 0;
                single_a[q + j] = oa ? a[j] : 0; single_b[q + j] = ob ? b[j] : 0;
            }
        }
        pair_wave_totals(kept, oa, ob, tot);
    }
}

}  // namespace tsx
