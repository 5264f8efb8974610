// tsx_normalize.h -- digital normalization (gfx950, wave64): records are judged round by round against the table as
// it stands, and only the k-mers of the records a round keeps are counted.
//
//   round_bounds_kernel     where the rounds of a text start (the first line of their first record)
//   normalize_keep_kernel   the rule per record of a round (median < cutoff): its keep bit, the bytes it contributes to
//                           the output, the round's totals
//   count_kept_kernel       count_fastq_kernel's tile loop with a record gate: a window is admitted when its record is
//                           one of the round's and its keep bit is set
// The medians come from window_counts_kernel and the select kernels (tsx_median.h) over the round's tiles and records.
#pragma once
#include "tsx_median.h"

namespace tsx {

enum { NT_KEPT = 0, NT_SEEN = 1, NT_ADDED = 2, NT_N = 3 };   // words of the totals

// out[j] = where record rec0 + j * R starts, for the nrounds rounds; out[nrounds] = end.  lo: trim_lines_kernel's.
__global__ __launch_bounds__(NT) void round_bounds_kernel(const unsigned long long *lo, uint64_t rec0, uint64_t R,
                                                          uint64_t nrounds, uint64_t end, unsigned long long *out) {
    for (uint64_t j = (uint64_t)blockIdx.x * NT + threadIdx.x; j <= nrounds; j += (uint64_t)gridDim.x * NT)
        out[j] = j < nrounds ? lo[(rec0 + j * R) * TL_N] : end;
}

// The records [rec0, rec1) of a round, after their medians: keep iff median < cutoff (a record without k-mers has
// median 0).  keep: one bit per record (zeroed before the first round; the bits of other rounds are not touched).
// len (with span; both may be NULL): the bytes record r contributes to the output, as filter_len_kernel leaves them --
// nl_last: record nrec_all - 1 lacks its '\n'.  keep_bytes (may be NULL): one byte per record < bytes_cap.
// totals[NT_*] grow by the round's kept records, k-mers seen and k-mers of kept records.
__global__ __launch_bounds__(NT) void normalize_keep_kernel(const unsigned long long *med, const unsigned long long *span,
                                                            uint64_t rec0, uint64_t rec1, uint64_t nrec_all, uint64_t cutoff,
                                                            int nl_last, uint32_t *keep, unsigned long long *len,
                                                            uint8_t *keep_bytes, uint64_t bytes_cap,
                                                            unsigned long long *totals) {
    const int lane = threadIdx.x & 63;
    unsigned long long kept = 0, seen = 0, added = 0;
    for (uint64_t r = rec0 + (uint64_t)blockIdx.x * NT + threadIdx.x; r < rec1; r += (uint64_t)gridDim.x * NT) {
        const uint64_t km = med[r * 2], md = med[r * 2 + 1];
        const bool k = md < cutoff;
        seen += km;
        if (k) {
            ++kept; added += km;
            atomicOr(keep + (r >> 5), 1u << (r & 31));
        }
        if (len) len[r] = k ? span[r * 2 + 1] - span[r * 2] + ((nl_last && r + 1 == nrec_all) ? 1 : 0) : 0;
        if (keep_bytes && r < bytes_cap) keep_bytes[r] = k ? 1 : 0;
    }
    for (int d = 32; d > 0; d >>= 1) {
        kept += __shfl_down(kept, d, 64); seen += __shfl_down(seen, d, 64); added += __shfl_down(added, d, 64);
    }
    if (lane == 0) {
        if (kept) atomicAdd(totals + NT_KEPT, kept);
        if (seen) atomicAdd(totals + NT_SEEN, seen);
        if (added) atomicAdd(totals + NT_ADDED, added);
    }
}

// Whether one of the records [ra, rb] has its keep bit set.  The same answer in every lane.
__device__ __forceinline__ bool any_kept(const uint32_t *keep, uint64_t ra, uint64_t rb) {
    for (uint64_t w = ra >> 5; w <= (rb >> 5); ++w) {
        uint32_t bits = keep[w];
        if (w == (ra >> 5)) bits &= ~0u << (ra & 31);
        if (w == (rb >> 5)) bits &= ~0u >> (31 - (rb & 31));
        if (bits) return true;
    }
    return false;
}

// count_fastq_kernel (tsx_kernels.h) over the tiles [tile0, tile_end) of a text that has had its line pass (tile_line:
// tiles_all entries), with a record gate.  The line index is kept whole and offset by *line_base, so the record of a
// window is (line_base + line) >> lshift, as in query_reads_kernel.  A valid window is ADMITTED when that record lies in
// [rec0, rec1) -- the round: the tiles at its ends hold records of the rounds next to it, whose bits may be set -- and
// its bit in `keep` is set.  Only admitted windows take part in the run merge, the LDS dedup and ST_KMERS.
//
// Runs and the gate: run_leader and run_length break a run at every lane that is not admitted.  The gate is constant
// over a record, and the windows of two records never sit in adjacent lanes: the last k - 1 start positions of a
// sequence line are invalid (their window holds the line's '\n'), and so is every position of the lines between two
// sequence lines.  So a run of equal k-mers that the gate lets through lies inside one kept record, and no count of a
// dropped record reaches a kept neighbour's run.
//
// A tile whose lines hold no kept record of the round is skipped before its loads (*skipped counts them): with deep
// coverage most records are dropped.
template <int WK, bool CANON = false, bool BR = false>
__global__ __launch_bounds__(NT, WK == 1 ? 3 : 2) void count_kept_kernel(TableParams p, const uint8_t *buf, uint64_t n,
                                                        uint64_t own_end, int head_open, const uint32_t *tile_line,
                                                        uint64_t tile0, uint64_t tile_end, uint64_t tiles_all,
                                                        const unsigned long long *line_base, uint32_t lshift,
                                                        const uint32_t *keep, uint64_t rec0, uint64_t rec1,
                                                        unsigned long long *skipped, const uint16_t *qmap = nullptr) {
    __shared__ TileLds<uint32_t> s;
    __shared__ uint32_t s_dpos[DSLOTS];
    __shared__ uint32_t s_dcnt[DSLOTS];
    extern __shared__ uint64_t s_lut[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int lut_words = p.groups * (1 << p.g) * WK;
    for (int i = tid; i < lut_words; i += NT) s_lut[i] = p.lut[i];
    for (int i = tid; i < DSLOTS; i += NT) { s_dpos[i] = 0; s_dcnt[i] = 0; }
    s.set_sentinels(tid);
    unsigned long long added = 0;
    uint32_t nskip = 0;
    const WindowRule rule(p, n, own_end, *line_base);
    for (uint64_t tile = tile0 + blockIdx.x; tile < tile_end; tile += gridDim.x) {
        {   // the records whose lines the tile touches, cut to the round (the same in every lane: no barrier is split)
            const uint64_t ra = max((rule.lbase + tile_line[tile]) >> lshift, rec0);
            const uint64_t rb = tile + 1 < tiles_all ? min((rule.lbase + tile_line[tile + 1]) >> lshift, rec1 - 1) : rec1 - 1;
            if (ra > rb || !any_kept(keep, ra, rb)) { ++nskip; continue; }
        }
        const uint64_t base = tile * TILE;
        lds_barrier();  // previous tile's LDS fully consumed
        tile_stage<BR>(s, tile_load(buf, n, head_open, tile_line, tile, tid), p, qmap, base, n, tid);
        lds_barrier();

        for (int round = 0; round < TILE / BATCH; ++round) {
            uint64_t hk[PER_THREAD][WK];
            int slot_of[PER_THREAD];      // >=0: claimed LDS slot, -1: nothing to insert, -2: direct
            uint32_t direct_cnt[PER_THREAD];
#pragma unroll
            for (int j = 0; j < PER_THREAD; ++j) {
                const uint32_t pp = (uint32_t)(round * BATCH + j * NT + tid);
                uint32_t line;
                bool valid = window_valid(s, rule, base, pp, line);
                if (valid) {   // the gate
                    const uint64_t rec = (rule.lbase + line) >> lshift;
                    valid = rec >= rec0 && rec < rec1 && ((keep[rec >> 5] >> (rec & 31)) & 1u);
                }
                slot_of[j] = -1; direct_cnt[j] = 0;
                if (__ballot(valid) == 0ULL) continue;
                uint64_t x[WK];
                extract_kmer<WK>(s.codes, pp, p.top_mask, x);
                const bool leader = run_leader<WK>(x, valid, lane);
                const uint32_t runlen = run_length(leader, valid, lane);
                added += valid ? 1ULL : 0ULL;
                if (leader) {
                    hash_key<CANON, WK>(p, (const uint64_t *)s_lut, x, hk[j]);
                    uint32_t slot = (uint32_t)(mix64(hk[j][0] ^ (WK > 1 ? hk[j][WK - 1] : 0)) >> 40) & (DSLOTS - 1);
                    slot_of[j] = -2; direct_cnt[j] = runlen;
                    for (int pr = 0; pr < DPROBES; ++pr) {
                        const uint32_t old = atomicCAS(&s_dpos[slot], 0u, pp + 1u);
                        if (old == 0u) {
                            atomicAdd(&s_dcnt[slot], runlen);
                            slot_of[j] = (int)slot;
                            break;
                        }
                        uint64_t y[WK];
                        extract_kmer<WK>(s.codes, old - 1u, p.top_mask, y);
                        if (kmer_eq<WK>(x, y)) {
                            atomicAdd(&s_dcnt[slot], runlen);
                            slot_of[j] = -1;
                            break;
                        }
                        slot = (slot + 1) & (DSLOTS - 1);
                    }
                }
            }
            lds_barrier();
            // the claimant of each dedup slot issues ONE global insert carrying the slot's total
#pragma unroll
            for (int j = 0; j < PER_THREAD; ++j) {
                if (slot_of[j] == -1) continue;
                uint64_t d = direct_cnt[j];
                if (slot_of[j] >= 0) {
                    d = s_dcnt[slot_of[j]];
                    s_dcnt[slot_of[j]] = 0;
                    s_dpos[slot_of[j]] = 0;
                }
                insert_key<WK>(p, hk[j], d);
            }
            lds_barrier();
        }
    }
    for (int d = 32; d > 0; d >>= 1) added += __shfl_down(added, d, 64);
    if (lane == 0 && added) atomicAdd(&p.stats[ST_KMERS], added);
    if (tid == 0 && nskip && skipped) atomicAdd(skipped, (unsigned long long)nskip);
}

}  // namespace tsx
