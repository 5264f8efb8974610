// tsx_baserule.h -- the base rule's low-quality bitmap (gfx950, wave64).  tsx_hip_set_base_rule.
//
// A window is a k-mer under min_qual_char only if every base in it has a quality byte >= min_qual_char.  A tile cannot
// see the quality line of its bases (it usually lies in another tile), so a pass of its own writes one bit per text
// byte -- laid out like the front ends' newline mask, 16 bytes to a 16-bit word -- and the scan front ends OR it into
// their break mask (rule_bits16, tsx_kernels.h).  Only bits of sequence-line bytes are ever set: every other byte is
// outside any window that counts, and the caller zeroes the bitmap first.
//
//   qual_lines_kernel  where the sequence line and the quality line of every record start and end, from the classify16
//                      masks and tile_line as record_scan_kernel (tsx_query.h) finds its spans
//   qual_bits_kernel   16 lanes per record: bit j of the sequence line = quality byte j is below min_qual_char or
//                      missing (a quality line shorter than the sequence); quality bytes past the sequence are ignored
//
// The text starts at a record boundary (line 0 is a header) and every record whose bases count lies wholly inside it:
// device texts are taken whole, host pieces and BGZF batches are cut at record boundaries (tsxcount_hip.hip).
#pragma once
#include "tsx_kernels.h"

namespace tsx {

enum { QR_SEQ0 = 0, QR_SEQ1 = 1, QR_QUAL0 = 2, QR_QUAL1 = 3, QR_N = 4 };   // per record: [start, end) of both lines

// After the line pass over [0, n) from line 0 (tile_line, *carry = line ends).  rec (QR_N words per record, zeroed
// by the caller: a record without a quality line keeps an empty one) is written for records r < nrec.
__global__ __launch_bounds__(NT) void qual_lines_kernel(const uint8_t *buf, uint64_t n, const uint32_t *tile_line,
                                                        uint64_t ntiles, const uint32_t *carry,
                                                        unsigned long long *rec, uint64_t nrec) {
    __shared__ uint32_t s_w[NT / 64];
    const int lane = threadIdx.x & 63;
    if (blockIdx.x == 0 && threadIdx.x == 0 && n > 0 && buf[n - 1] != (uint8_t)'\n') {   // an unterminated last line
        const uint64_t e = *carry;
        if ((e & 1u) && (e >> 2) < nrec) rec[(e >> 2) * QR_N + ((e & 2u) ? QR_QUAL1 : QR_SEQ1)] = n;
    }
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t off = tile * TILE + (uint64_t)threadIdx.x * 16;
        const bool pnl = prev_is_nl(buf, off, n, 0);
        uint32_t nl, le, code;
        classify16(load16(buf, off, n), pnl, nl, le, code);
        const uint32_t lim = (off + 16 > n) ? ((off >= n) ? 0u : ((1u << (n - off)) - 1u)) : 0xFFFFu;
        le &= lim;
        const uint32_t ls = ~nl & ((nl << 1) | (pnl ? 1u : 0u)) & lim;   // first bytes of non-empty lines
        const uint32_t c = __popc(le);
        const uint32_t inc = wave_incl_scan(c);
        if (lane == 63) s_w[threadIdx.x >> 6] = inc;
        __syncthreads();
        uint32_t woff = tile_line[tile];
        for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) woff += s_w[w];
        woff += inc - c;   // line ends before this lane's 16 bytes
        for (uint32_t b = le | ls; b; b &= b - 1) {
            const uint32_t i = __builtin_ctz(b);
            const uint64_t line = woff + __popc(le & ((1u << i) - 1u));   // the line this byte starts or ends
            if (!(line & 1u) || (line >> 2) >= nrec) continue;            // lines 1 and 3 of a record only
            const uint32_t f = ((line & 2u) ? QR_QUAL0 : QR_SEQ0) + (((le >> i) & 1u) ? 1u : 0u);
            rec[(line >> 2) * QR_N + f] = off + i;
        }
        __syncthreads();
    }
}

// 16 lanes per record, one 16-bit bitmap word per lane and step.  A word that lies wholly inside a sequence line is
// stored; the first and last word of a line may hold bytes of the record before or after it and are ORed atomically.
__global__ __launch_bounds__(NT) void qual_bits_kernel(const uint8_t *buf, const unsigned long long *rec, uint64_t nrec,
                                                       uint32_t min_qual, uint16_t *qmap) {
    const uint32_t sub = threadIdx.x & 15u;
    const uint64_t g0 = ((uint64_t)blockIdx.x * NT + threadIdx.x) >> 4, ng = ((uint64_t)gridDim.x * NT) >> 4;
    for (uint64_t r = g0; r < nrec; r += ng) {
        const unsigned long long *e = rec + r * QR_N;
        const uint64_t s0 = e[QR_SEQ0], s1 = e[QR_SEQ1], q0 = e[QR_QUAL0], q1 = e[QR_QUAL1];
        if (s1 <= s0) continue;   // no sequence line (a truncated last record)
        const uint64_t lq = (q1 > q0) ? q1 - q0 : 0;
        for (uint64_t w = (s0 >> 4) + sub; w <= ((s1 - 1) >> 4); w += 16) {
            const uint64_t b0 = w * 16;
            uint32_t bits = 0;
#pragma unroll 4
            for (uint32_t i = 0; i < 16u; ++i) {
                const uint64_t b = b0 + i;
                if (b < s0 || b >= s1) continue;
                const uint64_t j = b - s0;
                if (j >= lq || (uint32_t)buf[q0 + j] < min_qual) bits |= 1u << i;
            }
            if (b0 >= s0 && b0 + 16 <= s1) qmap[w] = (uint16_t)bits;
            else if (bits) atomicOr(reinterpret_cast<uint32_t *>(qmap) + (w >> 1), bits << (16u * (uint32_t)(w & 1u)));
        }
    }
}

}  // namespace tsx
