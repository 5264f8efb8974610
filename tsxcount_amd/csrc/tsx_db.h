// tsx_db.h -- the k-mer database kernels (gfx950, wave64): the occupied slots of a table in and out of the chunks of
// tsx_hip_save_host / tsx_hip_load_host (include/tsxcount_hip.h; the file format is DESIGN.md §3 "K-mer database").
//
// A chunk covers the slots [slot_lo, slot_hi) (slot_lo a multiple of 64): one bitmap word per 64 slots (bit j of word w
// = slot slot_lo + 64 w + j is occupied), then the W words of every occupied slot in slot order, exactly as the table
// holds them.  The work is cut into tiles of DB_TILE slots, one workgroup each; the place of a tile's first entry in
// the compacted array comes from a count pass and a one-workgroup scan (two passes over limb 0 instead of one kernel
// with a decoupled look-back: see DESIGN.md for why).
//
//   db_count_table_kernel   save, pass 1: occupied slots per tile
//   db_count_bitmap_kernel  load, pass 1: the same from the chunk's bitmap
//   db_scan_kernel          exclusive scan of the tile counts (the total lands behind them)
//   db_pack_kernel          save, pass 2: bitmap word = __ballot(limb 0 != 0) of a wave, compacted entries, checksum
//   db_load_kernel          load, pass 2: PLACE = expand bitmap + entries into the table's slots (the direct load), else
//                           turn each entry into its k-mer and in-slot count (the re-insert path, add_kmers_kernel next);
//                           both check every entry and sum the checksum of what they read
//   db_carry_gather_kernel  save: the secondary array's entries as self-contained carry records
//   db_carry_kernel         load: carry records into the secondary array (PLACE) or into k-mers with count carry << C
//
// Chunk checksum (mod 2^64, order-free so that any number of workgroups can add to it): for every bitmap word b of
// global word index g = slot_lo / 64 + w, mix64(mix64(g ^ DB_SALT_BM) ^ b); for every occupied slot pos with words
// e[0..W), h = mix64(pos ^ DB_SALT_E), h = mix64(h ^ e[t]) for t = 0..W-1, then h.  Both maps are bijective, so any
// change to one word or one entry changes the sum.
#pragma once
#include "tsx_kernels.h"

namespace tsx {

constexpr uint32_t DB_TILE = 4096;   // slots per workgroup (64 bitmap words; 16 rounds of NT slots)
constexpr uint64_t DB_SALT_BM = 0x6A09E667F3BCC909ULL, DB_SALT_E = 0xBB67AE8584CAA73BULL;
// Per-chunk result words of a load.  TOTAL: the bitmap's set bits, copied behind the scan; ZERO: entries whose in-slot
// count is 0, each of which needs a carry record.
enum DbRes { DB_RES_SUM = 0, DB_RES_BAD = 1, DB_RES_TOTAL = 2, DB_RES_ZERO = 3, DB_RES_N = 4 };

__device__ __forceinline__ uint64_t db_bm_term(uint64_t gword, uint64_t bm) { return mix64(mix64(gword ^ DB_SALT_BM) ^ bm); }
__device__ __forceinline__ uint64_t db_entry_term(uint64_t pos, const uint64_t (&e)[4], int W) {
    uint64_t h = mix64(pos ^ DB_SALT_E);
    for (int t = 0; t < W; ++t) h = mix64(h ^ e[t]);
    return h;
}
// What the W words of an occupied slot of a well-formed table look like: reprobe count 1 .. max_reprobes and no bit
// outside the fields -- limb 0 holds the reprobe count, min(F, K0 - R) func bits and the counter (LOCK clear), limbs
// 1..W-1 the func bits that spill, low bits first.  A stray bit would make direct placement keep a word that no lookup
// matches while the re-insert path (words_to_kmer masks it away) counts a k-mer.
__device__ __forceinline__ bool db_word_ok(const TableParams &p, const uint64_t (&e)[4]) {
    const uint64_t i = e[0] & ((1ULL << p.R) - 1ULL);
    const int f0 = min(p.F, p.K0 - p.R);
    const uint64_t keep0 = ((1ULL << (p.R + f0)) - 1ULL) | (~0ULL << p.cshift);
    bool ok = i != 0 && i <= p.max_reprobes && (e[0] & ~keep0) == 0;
    int spill = p.F - f0;
    for (int t = 1; t < p.W; ++t, spill -= 64) {
        const uint64_t keep = spill >= 64 ? ~0ULL : spill <= 0 ? 0ULL : (1ULL << spill) - 1ULL;
        ok = ok && (e[t] & ~keep) == 0;
    }
    return ok;
}
// Sum over the lanes of the workgroup, one atomic per wave.
__device__ __forceinline__ void db_add(unsigned long long *dst, unsigned long long v) {
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(dst, v);
}
// The entries before this wave's in the current round of NT slots, and the round's total (every wave passes here).
__device__ __forceinline__ uint32_t db_wave_before(uint32_t wc, uint32_t *s_cnt, uint32_t &total) {
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) s_cnt[wave] = wc;
    __syncthreads();
    uint32_t before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) {
        const uint32_t c = s_cnt[w];
        before += (w < wave) ? c : 0u;
        total += c;
    }
    __syncthreads();   // s_cnt is written again by the next round
    return before;
}

// tile_cnt[t] = occupied slots of tile t of [slot_lo, slot_hi); grid = tiles.
__global__ __launch_bounds__(NT) void db_count_table_kernel(TableParams p, uint64_t slot_lo, uint64_t slot_hi,
                                                            unsigned long long *tile_cnt) {
    __shared__ uint32_t s_cnt[NT / 64];
    const uint64_t t0 = slot_lo + (uint64_t)blockIdx.x * DB_TILE;
    uint32_t c = 0;
    for (uint32_t r = 0; r < DB_TILE; r += NT) {
        const uint64_t pos = t0 + r + threadIdx.x;
        c += (pos < slot_hi && p.table[pos * (uint64_t)p.W] != 0) ? 1u : 0u;
    }
    for (int d = 32; d > 0; d >>= 1) c += __shfl_down(c, d, 64);
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
        for (int w = 0; w < NT / 64; ++w) s += s_cnt[w];
        tile_cnt[blockIdx.x] = s;
    }
}

// tile_cnt[t] = set bits of the 64 bitmap words of tile t (nbm words in all); one wave per tile.
__global__ __launch_bounds__(NT) void db_count_bitmap_kernel(const uint64_t *bm, uint64_t nbm, uint64_t ntiles,
                                                             unsigned long long *tile_cnt) {
    const uint64_t t = (uint64_t)blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const uint64_t w = t * (DB_TILE / 64) + lane;
    unsigned long long c = (t < ntiles && w < nbm) ? (unsigned long long)__popcll(bm[w]) : 0ULL;
    for (int d = 32; d > 0; d >>= 1) c += __shfl_down(c, d, 64);
    if (lane == 0 && t < ntiles) tile_cnt[t] = c;
}

// In place: cnt[0..n) -> exclusive prefix sums, cnt[n] = the total.  One workgroup (n is a chunk's tile count).
__global__ __launch_bounds__(NT) void db_scan_kernel(unsigned long long *cnt, uint64_t n) {
    __shared__ unsigned long long s_w[NT / 64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    unsigned long long carry = 0;
    for (uint64_t base = 0; base < n; base += NT) {
        const uint64_t i = base + threadIdx.x;
        const unsigned long long v = i < n ? cnt[i] : 0ULL;
        const unsigned long long inc = wave_incl_scan64(v);
        if (lane == 63) s_w[wave] = inc;
        __syncthreads();
        unsigned long long before = carry, total = 0;
        for (int w = 0; w < NT / 64; ++w) {
            before += (w < wave) ? s_w[w] : 0ULL;
            total += s_w[w];
        }
        if (i < n) cnt[i] = before + inc - v;
        carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) cnt[n] = carry;
}

// Save, pass 2, over the tiles of [slot_lo, slot_hi): bitmap words to bm_out (one per 64 slots of the range), the W
// words of every occupied slot to ent_out[tile_off[tile] + ...] (ent_cap entries at most), the checksum added to *sum.
__global__ __launch_bounds__(NT) void db_pack_kernel(TableParams p, uint64_t slot_lo, uint64_t slot_hi,
                                                     const unsigned long long *tile_off, uint64_t *bm_out, uint64_t *ent_out,
                                                     uint64_t ent_cap, unsigned long long *sum) {
    __shared__ uint32_t s_cnt[NT / 64];
    const int lane = threadIdx.x & 63, W = p.W;
    const uint64_t lt = (1ULL << lane) - 1ULL;
    const uint64_t t0 = slot_lo + (uint64_t)blockIdx.x * DB_TILE;
    uint64_t at = tile_off[blockIdx.x];
    unsigned long long cs = 0;
    for (uint32_t r = 0; r < DB_TILE; r += NT) {
        const uint64_t pos = t0 + r + threadIdx.x;
        const uint64_t wpos = pos - lane;   // first slot of this wave's bitmap word
        uint64_t e[4] = {0, 0, 0, 0};
        if (pos < slot_hi) e[0] = p.table[pos * (uint64_t)W];
        const bool occ = e[0] != 0;
        const uint64_t bal = __ballot(occ);
        uint32_t total;
        const uint32_t before = db_wave_before((uint32_t)__popcll(bal), s_cnt, total);
        if (wpos < slot_hi && lane == 0) {
            bm_out[(wpos - slot_lo) >> 6] = bal;
            cs += db_bm_term(wpos >> 6, bal);
        }
        if (occ) {
            for (int t = 1; t < W; ++t) e[t] = p.table[pos * (uint64_t)W + t];
            const uint64_t idx = at + before + (uint64_t)__popcll(bal & lt);
            if (idx < ent_cap)
                for (int t = 0; t < W; ++t) ent_out[idx * W + t] = e[t];
            cs += db_entry_term(pos, e, W);
        }
        at += total;
    }
    db_add(sum, cs);
}

// Load, pass 2, over the tiles of one chunk [slot_lo, slot_hi) held in device memory (bm: its bitmap, ent: its n_ent
// entries).  src: the layout of the database (the table's own for PLACE).  res[DB_RES_SUM] += checksum of what was read,
// res[DB_RES_BAD] += malformed entries (a set bit past slot_hi or past n_ent entries, a word that no table holds),
// res[DB_RES_ZERO] += entries whose in-slot count is 0 (the host matches them with carry records).
//   PLACE   every slot of the range is written (zeros where the bitmap has none), seg_dirty set where entries land
//   !PLACE  entry i -> kmers_out[i] (the k-mer, WK words) and counts_out[i] (its in-slot count)
template <bool PLACE, int WK>
__global__ __launch_bounds__(NT) void db_load_kernel(TableParams p, TableParams src, uint64_t slot_lo, uint64_t slot_hi,
                                                     const uint64_t *bm, const uint64_t *ent, uint64_t n_ent,
                                                     const unsigned long long *tile_off, uint64_t *kmers_out,
                                                     uint64_t *counts_out, unsigned long long *res) {
    __shared__ uint32_t s_cnt[NT / 64];
    const int lane = threadIdx.x & 63, W = src.W;
    const uint64_t lt = (1ULL << lane) - 1ULL;
    const uint64_t t0 = slot_lo + (uint64_t)blockIdx.x * DB_TILE;
    uint64_t at = tile_off[blockIdx.x];
    unsigned long long cs = 0, bad = 0, zero = 0;
    for (uint32_t r = 0; r < DB_TILE; r += NT) {
        const uint64_t pos = t0 + r + threadIdx.x;
        const uint64_t wpos = pos - lane;
        const uint64_t bal = (wpos < slot_hi) ? bm[(wpos - slot_lo) >> 6] : 0ULL;   // (one address per wave)
        const bool bit = (bal >> lane) & 1ULL;
        const bool occ = bit && pos < slot_hi;
        if (bit && !occ) bad += 1;
        uint32_t total;
        const uint32_t before = db_wave_before((uint32_t)__popcll(bal), s_cnt, total);
        if (wpos < slot_hi && lane == 0) cs += db_bm_term(wpos >> 6, bal);
        uint64_t e[4] = {0, 0, 0, 0};
        bool ok = false;
        if (occ) {
            const uint64_t idx = at + before + (uint64_t)__popcll(bal & lt);
            if (idx < n_ent) {
                for (int t = 0; t < W; ++t) e[t] = ent[idx * W + t];
                cs += db_entry_term(pos, e, W);
                ok = db_word_ok(src, e);
                zero += (e[0] >> src.cshift) == 0 ? 1 : 0;
                if (ok && !PLACE) {
                    uint64_t x[WK];
                    words_to_kmer<WK>(src, pos, e, x);
#pragma unroll
                    for (int t = 0; t < WK; ++t) kmers_out[idx * WK + t] = x[t];
                    counts_out[idx] = e[0] >> src.cshift;
                }
            }
            if (!ok) bad += 1;
        }
        if (PLACE && pos < slot_hi) {
            for (int t = 0; t < W; ++t) p.table[pos * (uint64_t)W + t] = ok ? e[t] : 0ULL;
            if (ok) p.seg_dirty[pos >> p.S] = 1;   // idempotent plain store, as insert_key
        }
        at += total;
    }
    db_add(&res[DB_RES_SUM], cs);
    db_add(&res[DB_RES_BAD], bad);
    db_add(&res[DB_RES_ZERO], zero);
}

// Save: every occupied entry of the secondary array as a record (pos, carry, the W words of slot pos), at most cap of
// them, in no particular order; *n = the number found.
__global__ __launch_bounds__(NT) void db_carry_gather_kernel(TableParams p, uint64_t *rec, uint64_t cap, unsigned long long *n) {
    const uint64_t sslots = p.sec_mask + 1, slots = p.slot_mask + 1;
    const int W = p.W, RW = 2 + p.W;
    for (uint64_t i = (uint64_t)blockIdx.x * NT + threadIdx.x; i < sslots; i += (uint64_t)gridDim.x * NT) {
        const uint64_t key = p.sec_keys[i];
        if (key == 0 || key > slots) continue;
        const uint64_t at = atomicAdd(n, 1ULL);
        if (at >= cap) continue;
        const uint64_t pos = key - 1;
        rec[at * RW] = pos;
        rec[at * RW + 1] = p.sec_cnt[i];
        for (int t = 0; t < W; ++t) rec[at * RW + 2 + t] = p.table[pos * (uint64_t)W + t];
    }
}

// Load: n carry records (2 + src.W words each, checked on the host).  PLACE: carry added to the secondary array at pos
// (the table's own secondary insert; its size may differ from the database's).  Else record i -> kmers_out[i] and
// counts_out[i] = carry << C of the database.
template <bool PLACE, int WK>
__global__ __launch_bounds__(NT) void db_carry_kernel(TableParams p, TableParams src, const uint64_t *rec, uint64_t n,
                                                      uint64_t *kmers_out, uint64_t *counts_out) {
    const int W = src.W, RW = 2 + src.W;
    for (uint64_t i = (uint64_t)blockIdx.x * NT + threadIdx.x; i < n; i += (uint64_t)gridDim.x * NT) {
        const uint64_t pos = rec[i * RW], carry = rec[i * RW + 1];
        if (PLACE) {
            sec_add(p, pos, carry);
        } else {
            uint64_t e[4] = {0, 0, 0, 0}, x[WK];
            for (int t = 0; t < W; ++t) e[t] = rec[i * RW + 2 + t];
            words_to_kmer<WK>(src, pos, e, x);
#pragma unroll
            for (int t = 0; t < WK; ++t) kmers_out[i * WK + t] = x[t];
            counts_out[i] = carry << src.C;
        }
    }
}

}  // namespace tsx
