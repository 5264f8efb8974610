// tsx_unitig.h -- unitigs, the compacted de Bruijn graph of ONE table (gfx950, wave64): the kernels behind
// tsx_hip_unitig_stats, tsx_hip_unitigs_* and tsx_hip_write_unitigs_host (include/tsxcount_hip.h; DESIGN.md §3 "Unitigs").
//
// The nodes are the k-mers counted in lower..upper; on a canonical table a node stands for both strands.  An ORIENTED
// node is a node read as a string s: the slot's own string x (what the inverse mapping gives: the strand with the
// smaller hash), or on a canonical table rc(x) -- `flip` below says which.  succ(s) are the strings s[1:] + c that are
// nodes, pred(s) the strings c + s[:-1]; an edge s -> t is compactable when |succ(s)| = 1, |pred(t)| = 1 and t lies in
// another slot than s.  A unitig is a maximal chain of compactable edges.
//
//   unitig_degree_kernel   sweeps the slots in tiles as het_sweep_kernel does.  Per in-range slot it probes the SAME table
//                          for the 4 + 4 neighbour strings of x and writes one SIDE BYTE: bits 0..2 the out code, bits 3..5
//                          the in code (0 none, 1 + c the unique base c, 5 several), bit 7 in range.  The hash is linear with
//                          h(0) = 0, so h(x[1:] + c) = h(x >> 2) ^ HI_c and h(c + x[:-1]) = h(x << 2) ^ LO_c: one hash per
//                          side (two on a canonical table: the reverse complement of a neighbour is a neighbour of rc(x) on
//                          the other side) and three constants per end, made on the host.  Totals in the same pass.
//   unitig_walk_kernel     an oriented node with no compactable edge into it is a start (unitig_step backwards fails).  A
//                          start walks its chain forwards, one lookup per step, reading the next node's side byte at the
//                          slot the lookup reports; it counts the k-mers, sums the counts and marks every slot in the
//                          covered bitmap.  On a canonical table both ends of a chain are starts and the one with s1 <
//                          rc(sm) as text emits.  Emitted chains become records (wave ballot, one atomic per wave for the
//                          record index and one for the sequence offset: the lengths are scanned inside the wave).
//   unitig_cycle_kernel    the in-range slots no walk covered lie on isolated cycles.  Each walks forwards until it meets
//                          a slot below its own (another slot is the cut point) or comes back to itself (it is: emit).
//   unitig_spell_kernel    one lane per record walks kmers - 1 steps again and writes the bases as ASCII.
//
// EVERY walk is bounded by `bound` = nodes + 1 steps; a walk that runs into the bound, a neighbour the side byte promises
// and the table does not hold, or an uncovered slot that is on no cycle raises UT_ERROR, which the host turns into an
// error return: no loop here needs a consistent table in order to end.
#pragma once
#include "tsx_kernels.h"
#include "tsx_het.h"

namespace tsx {

constexpr uint32_t UNITIG_TILE = CB_TILE;   // consecutive slots a workgroup walks before it strides on

// the device totals: the first UT_PUBLIC words are tsx_hip_unitig_totals
enum UnitigTotalIdx {
    UT_NODES = 0, UT_UNITIGS = 1, UT_CIRCULAR = 2, UT_BASES = 3, UT_LONGEST = 4, UT_ISOLATED = 5, UT_TIPS = 6, UT_BRANCHING = 7,
    UT_SUM = 8, UT_DEGREE = 9, UT_PUBLIC = UT_DEGREE + 25, UT_ERROR = UT_PUBLIC, UT_N = UT_PUBLIC + 1
};

constexpr uint32_t SIDE_SEVERAL = 5, SIDE_IN_RANGE = 0x80;

struct UnitigRec {   // tsx_hip_unitig
    uint64_t offset, length, kmers, sum_count, circular;
};

struct UnitigArgs {
    uint64_t lower, upper;     // a k-mer counted outside [lower, upper] is absent
    uint64_t lo[4][4];         // LO_c = h(base c at position 0), c = 0 gives 0 (limbs >= WK are 0)
    uint64_t hi[4][4];         // HI_c = h(base c at position k - 1)
    uint64_t bound;            // steps a walk may take: nodes + 1
    int32_t sec;               // the table ever carried: counts need the secondary array
    int32_t top_shift;         // base k - 1: bits top_shift, top_shift + 1 of limb WK - 1
};

// y = x[1:] + A (the bases move down one place) and y = A + x[:-1] (up one place, the last base drops out)
template <int WK>
__device__ __forceinline__ void kmer_drop_first(const uint64_t (&x)[WK], uint64_t (&y)[WK]) {
#pragma unroll
    for (int t = 0; t < WK; ++t) y[t] = (x[t] >> 2) | (t + 1 < WK ? x[t + 1] << 62 : 0ULL);
}
template <int WK>
__device__ __forceinline__ void kmer_drop_last(const TableParams &p, const uint64_t (&x)[WK], uint64_t (&y)[WK]) {
#pragma unroll
    for (int t = WK - 1; t >= 0; --t) y[t] = (x[t] << 2) | (t > 0 ? x[t - 1] >> 62 : 0ULL);
    y[WK - 1] &= p.top_mask;
}

// The count of the k-mer in slot pos (occupied).
__device__ __forceinline__ uint64_t unitig_slot_count(const TableParams &p, const UnitigArgs &a, uint64_t pos) {
    return (p.table[pos * (uint64_t)p.W] >> p.cshift) + (a.sec ? sec_get(p, pos) << p.C : 0ULL);
}

// An oriented node: its string, the reverse complement of it (canonical tables only), its slot, and whether the slot's
// own string is the reverse complement.
template <int WK>
struct UnitigCursor {
    uint64_t s[WK], rs[WK];
    uint64_t pos;
    bool flip;
};

// The code of one side of an oriented node from its slot's side byte: (out ? out : in) of the string as it is read, with
// the base complemented when the slot holds the other strand.
__device__ __forceinline__ uint32_t unitig_side(uint32_t byte, bool out, bool flip) {
    const uint32_t code = (out != flip) ? (byte & 7u) : ((byte >> 3) & 7u);
    return (flip && code >= 1 && code <= 4) ? 5u - code : code;
}

// One step along a compactable edge: FWD from c.s to its successor, else to its predecessor.  false when there is none
// (c is unchanged); true: c is the neighbour and cnt its count.  err: the side byte names a neighbour the table lacks.
template <int WK, bool CANON, bool FWD>
__device__ __forceinline__ bool unitig_step(const TableParams &p, const UnitigArgs &a, const uint8_t *side, UnitigCursor<WK> &c,
                                            uint64_t &cnt, bool &err) {
    const uint32_t code = unitig_side(side[c.pos], FWD, c.flip);
    if (code < 1 || code > 4) return false;
    const uint64_t b = code - 1;
    uint64_t t[WK], rt[WK], h[WK];
    bool flip = false;
    if constexpr (FWD) {
        kmer_drop_first<WK>(c.s, t);
        t[WK - 1] |= b << a.top_shift;
    } else {
        kmer_drop_last<WK>(p, c.s, t);
        t[0] |= b;
    }
    hash_apply<WK>(p, p.lut, t, h);
    if constexpr (CANON) {
        uint64_t hr[WK];
        if constexpr (FWD) {
            kmer_drop_last<WK>(p, c.rs, rt);
            rt[0] |= 3ULL - b;
        } else {
            kmer_drop_first<WK>(c.rs, rt);
            rt[WK - 1] |= (3ULL - b) << a.top_shift;
        }
        hash_apply<WK>(p, p.lut, rt, hr);
        flip = key_less<WK>(hr, h);
        key_min<WK>(h, hr);
    } else {
#pragma unroll
        for (int i = 0; i < WK; ++i) rt[i] = 0;
    }
    uint64_t pos = ~0ULL;
    const uint64_t n = lookup_key<WK>(p, h, &pos, a.sec != 0);
    if (pos == ~0ULL) { err = true; return false; }
    if (pos == c.pos) return false;   // a self-loop or a hairpin: the same node
    const uint32_t back = unitig_side(side[pos], !FWD, flip);
    if (back < 1 || back > 4) return false;
#pragma unroll
    for (int i = 0; i < WK; ++i) { c.s[i] = t[i]; c.rs[i] = rt[i]; }
    c.pos = pos;
    c.flip = flip;
    cnt = n;
    return true;
}

// The cursor of slot pos read as its own string (flip = false) or as the reverse complement (flip = true, canonical).
template <int WK, bool CANON>
__device__ __forceinline__ void unitig_cursor_at(const TableParams &p, uint64_t pos, bool flip, UnitigCursor<WK> &c) {
    uint64_t e[4] = {0, 0, 0, 0}, key[WK], x[WK], rx[WK];
    for (int t = 0; t < p.W; ++t) e[t] = p.table[pos * (uint64_t)p.W + t];
    words_to_key<WK>(p, pos, e, key);
    hash_apply<WK>(p, p.ilut, key, x);
    if constexpr (CANON) {
        revcomp<WK>(x, p.n, rx);
    } else {
#pragma unroll
        for (int t = 0; t < WK; ++t) rx[t] = 0;
    }
#pragma unroll
    for (int t = 0; t < WK; ++t) { c.s[t] = flip ? rx[t] : x[t]; c.rs[t] = flip ? x[t] : rx[t]; }
    c.pos = pos;
    c.flip = flip;
}

// Inclusive scan of v over the lanes of the wave.
__device__ __forceinline__ uint64_t unitig_wave_scan(uint64_t v, int lane) {
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t o = __shfl_up(v, d, 64);
        if (lane >= d) v += o;
    }
    return v;
}

// One record per lane with `emit` (all lanes of the wave call this): its index from tot[UT_UNITIGS], its offset from
// tot[UT_BASES], the longest into tot[UT_LONGEST].  Written for index < cap; start[index] = slot | flip << 63.
__device__ __forceinline__ void unitig_emit(bool emit, uint64_t kmers, uint64_t sum, bool circular, uint64_t start_word, int k,
                                            unsigned long long *tot, UnitigRec *rec, uint64_t *start, uint64_t cap) {
    const uint64_t grp = __ballot(emit);
    if (grp == 0) return;   // (wave-uniform)
    const int lane = threadIdx.x & 63;
    const uint64_t len = emit ? kmers + (uint64_t)k - 1 : 0ULL;
    const uint64_t upto = unitig_wave_scan(len, lane);
    uint64_t longest = len;
    for (int d = 32; d > 0; d >>= 1) { const uint64_t o = __shfl_down(longest, d, 64); longest = o > longest ? o : longest; }
    const int lead = __ffsll((long long)grp) - 1, last = 63;
    const uint64_t total = __shfl(upto, last, 64);
    unsigned long long at = 0, off = 0;
    if (lane == lead) {
        at = atomicAdd(&tot[UT_UNITIGS], (unsigned long long)__popcll(grp));
        off = atomicAdd(&tot[UT_BASES], (unsigned long long)total);
        if (circular) atomicAdd(&tot[UT_CIRCULAR], (unsigned long long)__popcll(grp));
    }
    if (lane == 0) atomicMax(&tot[UT_LONGEST], (unsigned long long)longest);
    at = __shfl(at, lead, 64) + (unsigned long long)__popcll(grp & ((1ULL << lane) - 1ULL));
    off = __shfl(off, lead, 64) + (upto - len);
    if (emit && at < cap) {
        rec[at] = UnitigRec{off, len, kmers, sum, circular ? 1ULL : 0ULL};
        start[at] = start_word;
    }
}

// Stage 1.  side: one byte per slot (every slot of the sweep is written); tot zeroed by the caller.  The host picks the
// grid so that no workgroup sweeps 2^31 slots or more (the per-lane sums are u32).
template <int WK, bool CANON>
__global__ __launch_bounds__(NT) void unitig_degree_kernel(TableParams p, UnitigArgs a, uint64_t slots, uint8_t *side,
                                                            unsigned long long *tot) {
    __shared__ unsigned long long s_tot[UT_PUBLIC];
    if (threadIdx.x < UT_PUBLIC) s_tot[threadIdx.x] = 0;
    __syncthreads();
    const int W = p.W;
    const int lane = threadIdx.x & 63;
    uint32_t n_nodes = 0, n_iso = 0, n_tips = 0, n_branch = 0;
    unsigned long long n_sum = 0;
    for (uint64_t t0 = (uint64_t)blockIdx.x * UNITIG_TILE; t0 < slots; t0 += (uint64_t)gridDim.x * UNITIG_TILE) {
        for (uint32_t r = 0; r < UNITIG_TILE; r += NT) {
            const uint64_t pos = t0 + r + threadIdx.x;
            uint64_t e[4] = {0, 0, 0, 0};
            if (pos < slots) e[0] = p.table[pos * (uint64_t)W];
            uint64_t sp = 0;
            if (e[0] != 0) sp = (e[0] >> p.cshift) + (a.sec ? sec_get(p, pos) << p.C : 0ULL);
            const bool in = sp != 0 && sp >= a.lower && sp <= a.upper;
            uint32_t byte = 0;
            if (in) {
                for (int t = 1; t < W; ++t) e[t] = p.table[pos * (uint64_t)W + t];
                uint64_t key[WK], x[WK], rx[WK], y[WK];
                words_to_key<WK>(p, pos, e, key);
                hash_apply<WK>(p, p.ilut, key, x);
                // hs[0] = h(x[1:] + A), hs[1] = h(A + x[:-1]); canonical: hr[0] = h(rc of a successor less its first base's
                // term) = h(A + rc(x)[:-1]), hr[1] = h(rc(x)[1:] + A)
                uint64_t hs[2][WK], hr[2][WK];
                kmer_drop_first<WK>(x, y);
                hash_apply<WK>(p, p.lut, y, hs[0]);
                kmer_drop_last<WK>(p, x, y);
                hash_apply<WK>(p, p.lut, y, hs[1]);
                bool swap = false;   // the strand a dump reports is rc(x): its in side is the out side of x
                if constexpr (CANON) {
                    revcomp<WK>(x, p.n, rx);
                    kmer_drop_last<WK>(p, rx, y);
                    hash_apply<WK>(p, p.lut, y, hr[0]);
                    kmer_drop_first<WK>(rx, y);
                    hash_apply<WK>(p, p.lut, y, hr[1]);
                    swap = kmer_text_less<WK>(rx, x);
                }
                uint32_t deg[2] = {0, 0}, code[2] = {0, 0};
#pragma unroll
                for (int sd = 0; sd < 2; ++sd) {       // 0: successors x[1:] + c, 1: predecessors c + x[:-1]
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        uint64_t q[WK];
#pragma unroll
                        for (int t = 0; t < WK; ++t) q[t] = hs[sd][t] ^ (sd == 0 ? a.hi[c][t] : a.lo[c][t]);
                        if constexpr (CANON) {
                            uint64_t o[WK];
#pragma unroll
                            for (int t = 0; t < WK; ++t) o[t] = hr[sd][t] ^ (sd == 0 ? a.lo[3 - c][t] : a.hi[3 - c][t]);
                            key_min<WK>(q, o);
                        }
                        const uint64_t n = lookup_key<WK>(p, q, nullptr, a.sec != 0);
                        if (n != 0 && n >= a.lower && n <= a.upper) {
                            ++deg[sd];
                            code[sd] = 1u + (uint32_t)c;
                        }
                    }
                    if (deg[sd] > 1) code[sd] = SIDE_SEVERAL;
                }
                byte = SIDE_IN_RANGE | code[0] | (code[1] << 3);
                const uint32_t dout = swap ? deg[1] : deg[0], din = swap ? deg[0] : deg[1];
                atomicAdd(&s_tot[UT_DEGREE + din * 5 + dout], 1ULL);
                ++n_nodes;
                n_sum += sp;
                n_iso += (din == 0 && dout == 0) ? 1u : 0u;
                n_tips += ((din == 0) != (dout == 0)) ? 1u : 0u;
                n_branch += (din > 1 || dout > 1) ? 1u : 0u;
            }
            if (pos < slots) side[pos] = (uint8_t)byte;
        }
    }
    unsigned long long v[5] = {n_nodes, n_iso, n_tips, n_branch, n_sum};
    const int at[5] = {UT_NODES, UT_ISOLATED, UT_TIPS, UT_BRANCHING, UT_SUM};
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        for (int d = 32; d > 0; d >>= 1) v[i] += __shfl_down(v[i], d, 64);
        if (lane == 0 && v[i]) atomicAdd(&s_tot[at[i]], v[i]);
    }
    __syncthreads();
    if (threadIdx.x < UT_PUBLIC && s_tot[threadIdx.x]) atomicAdd(&tot[threadIdx.x], s_tot[threadIdx.x]);
}

// Stage 2.  covered: one bit per slot, zeroed by the caller.  rec / start may be null with cap = 0 (totals only).
template <int WK, bool CANON>
__global__ __launch_bounds__(NT) void unitig_walk_kernel(TableParams p, UnitigArgs a, uint64_t slots, const uint8_t *side,
                                                          uint32_t *covered, unsigned long long *tot, UnitigRec *rec, uint64_t *start,
                                                          uint64_t cap) {
    for (uint64_t t0 = (uint64_t)blockIdx.x * UNITIG_TILE; t0 < slots; t0 += (uint64_t)gridDim.x * UNITIG_TILE) {
        for (uint32_t r = 0; r < UNITIG_TILE; r += NT) {
            const uint64_t pos = t0 + r + threadIdx.x;
            const bool in = pos < slots && (side[pos] & SIDE_IN_RANGE);
            bool emit = false, err = false;
            uint64_t kmers = 0, sum = 0, start_word = 0;
            if (in) {
                for (int o = 0; o < (CANON ? 2 : 1) && !emit; ++o) {
                    UnitigCursor<WK> c, back;
                    unitig_cursor_at<WK, CANON>(p, pos, o != 0, c);
                    back = c;
                    uint64_t n = 0;
                    if (unitig_step<WK, CANON, false>(p, a, side, back, n, err)) continue;   // a compactable edge comes in
                    uint64_t s1[WK];
#pragma unroll
                    for (int t = 0; t < WK; ++t) s1[t] = c.s[t];
                    uint64_t m = 1, total = unitig_slot_count(p, a, pos), steps = 0;
                    atomicOr(&covered[pos >> 5], 1u << (pos & 31));
                    while (unitig_step<WK, CANON, true>(p, a, side, c, n, err)) {
                        ++m;
                        total += n;
                        atomicOr(&covered[c.pos >> 5], 1u << (c.pos & 31));
                        if (++steps >= a.bound) { err = true; break; }
                    }
                    bool mine = true;
                    if constexpr (CANON) mine = kmer_text_less<WK>(s1, c.rs);   // s1 < rc(sm): the smaller spelling starts here
                    if (mine) {
                        emit = true;
                        kmers = m;
                        sum = total;
                        start_word = pos | (o ? 1ULL << 63 : 0ULL);
                    }
                }
            }
            if (err) atomicOr(&tot[UT_ERROR], 1ULL);
            unitig_emit(emit, kmers, sum, false, start_word, p.k, tot, rec, start, cap);
        }
    }
}

// Stage 4.  The in-range slots stage 2 left uncovered.
template <int WK, bool CANON>
__global__ __launch_bounds__(NT) void unitig_cycle_kernel(TableParams p, UnitigArgs a, uint64_t slots, const uint8_t *side,
                                                           const uint32_t *covered, unsigned long long *tot, UnitigRec *rec,
                                                           uint64_t *start, uint64_t cap) {
    for (uint64_t t0 = (uint64_t)blockIdx.x * UNITIG_TILE; t0 < slots; t0 += (uint64_t)gridDim.x * UNITIG_TILE) {
        for (uint32_t r = 0; r < UNITIG_TILE; r += NT) {
            const uint64_t pos = t0 + r + threadIdx.x;
            const bool todo = pos < slots && (side[pos] & SIDE_IN_RANGE) && !((covered[pos >> 5] >> (pos & 31)) & 1u);
            bool emit = false, err = false;
            uint64_t kmers = 0, sum = 0;
            if (todo) {
                UnitigCursor<WK> c;
                unitig_cursor_at<WK, CANON>(p, pos, false, c);
                uint64_t m = 1, total = unitig_slot_count(p, a, pos), n = 0, steps = 0;
                for (;;) {
                    if (!unitig_step<WK, CANON, true>(p, a, side, c, n, err) || ++steps >= a.bound) { err = true; break; }
                    if (c.pos == pos) { emit = !c.flip; err = c.flip; break; }
                    if (c.pos < pos) break;
                    ++m;
                    total += n;
                }
                kmers = m;
                sum = total;
            }
            if (err) atomicOr(&tot[UT_ERROR], 1ULL);
            unitig_emit(emit, kmers, sum, true, pos, p.k, tot, rec, start, cap);
        }
    }
}

// Stage 3.  Record r < n: its bases as ASCII at seq[offset, offset + length); the host has checked that every record ends
// inside the buffer (the offsets tile [0, tot[UT_BASES]) and that fits).  The walk takes kmers - 1 steps, whatever it meets.
template <int WK, bool CANON>
__global__ __launch_bounds__(NT) void unitig_spell_kernel(TableParams p, UnitigArgs a, const uint8_t *side, const UnitigRec *rec,
                                                           const uint64_t *start, uint64_t n, uint64_t seq_cap, uint8_t *seq,
                                                           unsigned long long *tot) {
    for (uint64_t r = (uint64_t)blockIdx.x * NT + threadIdx.x; r < n; r += (uint64_t)gridDim.x * NT) {
        const UnitigRec u = rec[r];
        if (u.offset > seq_cap || u.length > seq_cap - u.offset || u.length != u.kmers + (uint64_t)p.k - 1) {
            atomicOr(&tot[UT_ERROR], 1ULL);
            continue;
        }
        UnitigCursor<WK> c;
        unitig_cursor_at<WK, CANON>(p, start[r] & ~(1ULL << 63), (start[r] >> 63) != 0, c);
        uint8_t *out = seq + u.offset;
        uint64_t y[WK];
#pragma unroll
        for (int t = 0; t < WK; ++t) y[t] = c.s[t];
        for (int i = 0; i < p.k; ++i) {   // base i is the lowest one after i shifts (no runtime index into registers)
            out[i] = (uint8_t)(0x54474341u >> (8 * (uint32_t)(y[0] & 3ULL)));
            uint64_t z[WK];
            kmer_drop_first<WK>(y, z);
#pragma unroll
            for (int t = 0; t < WK; ++t) y[t] = z[t];
        }
        bool err = false;
        uint64_t cnt = 0;
        for (uint64_t i = 1; i < u.kmers; ++i) {
            if (!unitig_step<WK, CANON, true>(p, a, side, c, cnt, err)) { err = true; break; }
            out[(uint64_t)p.k - 1 + i] = (uint8_t)(0x54474341u >> (8 * (uint32_t)((c.s[WK - 1] >> a.top_shift) & 3ULL)));
        }
        if (err) atomicOr(&tot[UT_ERROR], 1ULL);
    }
}

}  // namespace tsx
