// tsx_track.h -- k-mer coverage tracks: the sequences of a wrapped FASTA in bins of W start positions (gfx950, wave64).
//
// The piece driver, the unwrap and the carries are those of tsx_seq.h.  Bin b of a sequence covers the start positions
// [b * W, (b + 1) * W) of the joined sequence; the bin rows of a piece are dense per record: record r owns
// ceil((off_r + len_r) / W) - floor(off_r / W) rows, off_r being the sequence coordinate of the first byte of its
// sequence line (0 but for a record 0 that goes on with an open sequence: row0_off, the bases in front of the piece minus
// those carried in) and len_r the length of that line.
//
//   track_rows_kernel     rows per record out of its span; the u64 scan kernels of tsx_query.h make the exclusive prefix
//   seq_track_kernel      the tile front end and the lookup schedule of seq_stats_kernel; a run is (wave row, record, bin);
//                         the runs of a tile are folded in LDS by bin row and leave the tile as one set of global atomics
//                         per bin it touches
//   track_finalize_kernel min_count back out of ~min, min_count and max_count of bins without k-mers 0
//
// Where the bin of a position comes from: ONE 64-bit division per tile, for the tile's first position.  From there on
// every dividend is below W + TILE (a position of the record at the tile's first byte: the remainder of that division
// plus the offset in the tile) or below TILE (a record that starts in the tile starts at coordinate 0), so the quotient
// is a compare when W >= TILE and a 32-bit multiply by 2^32 / W + 1 when not (track_div).  Only the first lane of a
// (wave row, record) run does that; W >= 64 lets the lanes behind it find their bin by a compare: the run crosses at most
// one bin border.
//
// Row layout: five uint64 per bin {kmers, present, min_count, max_count, sum_count} (tsx_hip_seq_bin).
#pragma once
#include "tsx_seq.h"

namespace tsx {

enum { TB_KMERS = 0, TB_PRESENT = 1, TB_MIN = 2, TB_MAX = 3, TB_SUM = 4, TB_N = 5 };
constexpr int TRACK_FOLD = NT;           // bin rows of a tile that fold in LDS (one slot per thread); the rest go to HBM
constexpr uint32_t TRACK_DROP = 0xFFFFFFFFu;   // the row of a run whose record lies past the piece's records

struct TrackFold {
    uint32_t kmers[TRACK_FOLD], present[TRACK_FOLD];
    unsigned long long sum[TRACK_FOLD], nmin[TRACK_FOLD], mx[TRACK_FOLD];   // nmin: ~min under max
};

// t / W for t < W + TILE (t < 2 * TILE when W < TILE), magic = 2^32 / W + 1: with e = magic * W - 2^32 <= W < 2^12 and
// t < 2^13 the product t * e stays below 2^32, which makes the high word of t * magic the exact quotient.
__device__ __forceinline__ uint32_t track_div(uint64_t t, uint64_t W, uint32_t magic, uint64_t &rem) {
    const uint32_t q = (W >= (uint64_t)TILE) ? (t >= W ? 1u : 0u) : __umulhi((uint32_t)t, magic);
    rem = t - (uint64_t)q * W;
    return q;
}

// cnt[r] = the bin rows of record r (cnt has nrec + 1 entries, the last 0: the scan leaves the total there).
__global__ __launch_bounds__(NT) void track_rows_kernel(const unsigned long long *span, uint64_t nrec, uint64_t W,
                                                        uint64_t row0_off, unsigned long long *cnt) {
    for (uint64_t r = (uint64_t)blockIdx.x * NT + threadIdx.x; r <= nrec; r += (uint64_t)gridDim.x * NT) {
        unsigned long long c = 0;
        if (r < nrec) {
            const uint64_t off = r == 0 ? row0_off : 0ULL, len = span[r * 2 + 1] - span[r * 2] - 3;
            c = (off + len + W - 1) / W - off / W;
        }
        cnt[r] = c;
    }
}

// Tiles [0, ntiles) of the unwrapped piece buf[0, n), as seq_stats_kernel.  bins: TB_N words per bin row of the piece,
// zeroed, rows >= bin_cap are dropped; row_of: the exclusive prefix of track_rows_kernel; W: the window, magic: 2^32 / W
// + 1 (track_div), off0_bin: row0_off / W.
template <int WK, bool CANON = false, bool BR = false>
__global__ __launch_bounds__(NT, 2) void seq_track_kernel(TableParams p, const uint8_t *buf, uint64_t n, const uint32_t *tile_line,
                                                          uint64_t ntiles, const unsigned long long *line_base, uint64_t lower,
                                                          uint64_t upper, unsigned long long *bins, uint64_t bin_cap, uint64_t nrec,
                                                          const unsigned long long *span, const unsigned long long *row_of,
                                                          uint64_t W, uint32_t magic, uint64_t row0_off, uint64_t off0_bin) {
    __shared__ TileLds<uint32_t> s;
    __shared__ TrackFold f;
    extern __shared__ uint64_t s_lut[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int lut_words = p.groups * (1 << p.g) * WK;
    for (int i = tid; i < lut_words; i += NT) s_lut[i] = p.lut[i];
    s.set_sentinels(tid);
    const WindowRule rule(p, n, n, *line_base);
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t base = tile * TILE;
        lds_barrier();  // previous tile's LDS fully consumed (its fold flushed)
        const TileText tt = tile_load(buf, n, 0, tile_line, tile, tid);
        tile_stage<BR>(s, tt, p, (const uint16_t *)nullptr, base, n, tid);
        f.kmers[tid] = 0; f.present[tid] = 0; f.sum[tid] = 0; f.nmin[tid] = 0; f.mx[tid] = 0;
        lds_barrier();
        // the record at the tile's first byte and the bin of its first sequence position at or behind that byte: no run
        // of the tile lies in a row below row00; rb: that position's offset in its bin, p_first: its offset in the tile
        const uint64_t rec0 = (rule.lbase + tt.line) >> 1;
        uint64_t row00 = 0, rb = 0;
        uint32_t p_first = 0;
        if (rec0 < nrec) {
            const uint64_t s0 = span[rec0 * 2] + 2, off0 = rec0 == 0 ? row0_off : 0ULL;
            const uint64_t x0 = (base > s0 ? base - s0 : 0ULL) + off0, q0 = x0 / W;
            p_first = s0 > base ? (uint32_t)(s0 - base) : 0u;
            rb = x0 - q0 * W;
            row00 = row_of[rec0] + q0 - (rec0 == 0 ? off0_bin : 0ULL);
        }

        for (int round = 0; round < TILE / BATCH; ++round) {
            ProbeRound<WK> pr;
            probe_round_issue<CANON, WK>(p, (const uint64_t *)s_lut, s, rule, base, round, tid, pr);
#pragma unroll
            for (int j = 0; j < PER_THREAD; ++j) {
                const bool valid = (pr.vbits >> j) & 1u;
                uint64_t c;
                const unsigned long long vmask = probe_round_count<WK>(p, pr, j, lane, c);
                if (vmask == 0ULL) continue;
                const uint32_t pp = (uint32_t)(round * BATCH + j * NT + tid);
                // the first lane of a (wave row, record) run: its row relative to row00 and its offset in that bin
                const bool rhead = valid && (lane == 0 || !((vmask >> (lane - 1)) & 1ULL));
                uint32_t rel = TRACK_DROP, rem = 0;
                if (rhead) {
                    const uint64_t rec = (rule.lbase + tile_line_of(s, pp)) >> 1;
                    if (rec < nrec) {
                        uint64_t t, r0 = 0, rm;
                        if (rec == rec0) {
                            t = rb + (uint64_t)(pp - p_first);
                        } else {   // (a record that starts in the tile: rec > 0, its coordinates start at 0)
                            t = base + pp - (span[rec * 2] + 2);
                            r0 = row_of[rec] - row00;
                        }
                        rel = (uint32_t)r0 + track_div(t, W, magic, rm);
                        rem = (uint32_t)rm;
                    }
                }
                // the lanes behind it: W >= 64 puts at most one bin border into the run
                const unsigned long long rmask = __ballot(rhead) & (~0ULL >> (63 - lane));   // run heads at or below the lane
                const int src = rmask ? 63 - __builtin_clzll(rmask) : lane;
                const uint32_t rel_h = __shfl(rel, src, 64), rem_h = __shfl(rem, src, 64);
                const uint64_t t2 = (uint64_t)rem_h + (uint64_t)(lane - src);
                const bool use = valid && rel_h != TRACK_DROP;
                const uint32_t row = rel_h + (t2 >= W ? 1u : 0u);
                const bool head = use && (rhead || t2 == W);
                const uint32_t seg = run_length(head, use, lane);
                const bool in = use && c >= lower && c <= upper;
                unsigned long long sum = use ? c : 0ULL, mn = use ? c : ~0ULL, mx = use ? c : 0ULL;
                uint32_t inr = in ? 1u : 0u;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const unsigned long long os = __shfl_down(sum, d, 64), om = __shfl_down(mn, d, 64), ox = __shfl_down(mx, d, 64);
                    const uint32_t oi = __shfl_down(inr, d, 64);
                    if ((uint32_t)d < seg) { sum += os; mn = om < mn ? om : mn; mx = ox > mx ? ox : mx; inr += oi; }
                }
                if (head) {
                    if (row < (uint32_t)TRACK_FOLD) {
                        atomicAdd(&f.kmers[row], seg);
                        if (inr) atomicAdd(&f.present[row], inr);
                        atomicAdd(&f.sum[row], sum);
                        atomicMax(&f.nmin[row], ~mn);
                        atomicMax(&f.mx[row], mx);
                    } else if (row00 + row < bin_cap) {   // a tile of more than TRACK_FOLD bin rows (many tiny records)
                        unsigned long long *st = bins + (row00 + row) * TB_N;
                        atomicAdd(st + TB_KMERS, (unsigned long long)seg);
                        if (inr) atomicAdd(st + TB_PRESENT, (unsigned long long)inr);
                        atomicAdd(st + TB_SUM, sum);
                        atomicMax(st + TB_MIN, ~mn);
                        atomicMax(st + TB_MAX, mx);
                    }
                }
            }
        }
        lds_barrier();
        if (f.kmers[tid] && row00 + tid < bin_cap) {
            unsigned long long *st = bins + (row00 + tid) * TB_N;
            atomicAdd(st + TB_KMERS, (unsigned long long)f.kmers[tid]);
            if (f.present[tid]) atomicAdd(st + TB_PRESENT, (unsigned long long)f.present[tid]);
            atomicAdd(st + TB_SUM, f.sum[tid]);
            atomicMax(st + TB_MIN, f.nmin[tid]);
            atomicMax(st + TB_MAX, f.mx[tid]);
        }
    }
}

// min_count = ~(the max of ~c); min_count and max_count 0 without k-mers.  Rows [0, min(*total, cap)).
__global__ __launch_bounds__(NT) void track_finalize_kernel(unsigned long long *bins, const unsigned long long *total, uint64_t cap) {
    const uint64_t lim = min((uint64_t)*total, cap);
    for (uint64_t r = (uint64_t)blockIdx.x * NT + threadIdx.x; r < lim; r += (uint64_t)gridDim.x * NT) {
        unsigned long long *s = bins + r * TB_N;
        const bool any = s[TB_KMERS] != 0;
        s[TB_MIN] = any ? ~s[TB_MIN] : 0ULL;
        s[TB_MAX] = any ? s[TB_MAX] : 0ULL;
    }
}

}  // namespace tsx
