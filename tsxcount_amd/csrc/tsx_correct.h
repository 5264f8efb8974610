// tsx_correct.h -- read error correction (gfx950, wave64): single substitutions undone from the k-mer spectrum; the
// kernels behind tsx_hip_correct_* (include/tsxcount_hip.h; DESIGN.md §3 "Read correction").
//
// The solid bitmap (solid_bits_kernel) and the line offsets (trim_lines_kernel) are those of the trim (tsx_trim.h).
//   correct_sites_kernel   the maximal runs of non-solid windows of every record, from its stretch of the bitmap; the runs
//                          the rule calls sites go to a list (record, a, w, p)
//   correct_probe_kernel   one site per wave: lane i hashes window a + i once; the key of "that window with base p
//                          changed by d" is the key XOR a constant, so the three alternatives cost three probes and no
//                          hash; ballots reduce the verdicts, one lane writes the correction
//   correct_apply_kernel   the `to` bytes into the output copy of the text, one lane per correction
//
// The constant: the hash is GF(2)-linear (tsx_het.h), so h(x ^ (d << 2j)) = h(x) ^ A * (d << 2j), and A * (d << 2j) is
// the LUT's own entry [group of bit 2j][d << (2j - the group's first bit)] -- a 2-bit field never straddles a group of 4
// or 8 bits.  The k x 3 constants are read from the LUT the kernel stages in LDS anyway; no second table is made.
// Canonical tables: rc(x ^ (d << 2j)) = rc(x) ^ (d << 2(k - 1 - j)) (the complement is XOR 3 on the code), so with
// hr = h(rc x) alternative d's key is min(h ^ H[j][d], hr ^ H[k - 1 - j][d]).
#pragma once
#include "tsx_trim.h"

namespace tsx {

struct CorrectSite {
    uint64_t rec;       // record of the lo array
    uint32_t a, w, p;   // first window and windows of the run, the suspect base (offsets in the sequence line)
    uint32_t pad;
};
// tsx_hip_correction
struct CorrectionRec {
    uint64_t record;
    uint32_t pos;
    uint8_t from, to;
    uint16_t windows;
};
static_assert(sizeof(CorrectSite) == 24 && sizeof(CorrectionRec) == 16, "site and correction records");

enum CorrectTotIdx { CT_CORRECTED = 0, CT_AMBIGUOUS = 1, CT_UNFIXABLE = 2, CT_N = 3 };

constexpr uint32_t CORRECT_LONG_WORDS = 64;   // a record with more bitmap words than this is walked by its whole wave

// Every run of non-solid windows of the record with windows [G0, G1) (bit positions; G1 - G0 >= 2) that ENDS in bitmap
// word wi (a word that holds one of them): its start is found by walking back, at most until the run is longer than k
// (no site then), and the sites among them are appended.
__device__ __forceinline__ void correct_word_runs(const unsigned long long *bits, uint64_t wi, uint64_t G0, uint64_t G1,
                                                  uint32_t k, uint32_t minw, uint64_t rec, CorrectSite *sites,
                                                  uint64_t site_cap, unsigned long long *n_sites) {
    const uint64_t wlo = wi * 64;
    unsigned long long z = ~bits[wi];
    if (G0 > wlo) z &= ~0ULL << (G0 - wlo);
    if (G1 < wlo + 64) z &= (1ULL << (G1 - wlo)) - 1ULL;
    if (z == 0) return;
    const unsigned long long nx = (wlo + 64 < G1) ? (~bits[wi + 1] & 1ULL) : 0ULL;   // window wlo + 64 is non-solid
    for (unsigned long long ends = z & ~((z >> 1) | (nx << 63)); ends; ends &= ends - 1) {
        const uint32_t e = (uint32_t)__builtin_ctzll(ends);
        const uint64_t b = wlo + e;
        const unsigned long long gaps = e ? (~z & ((1ULL << e) - 1ULL)) : 0ULL;   // solid (or outside) below the end
        uint64_t a;
        if (gaps) {
            a = wlo + 64 - (uint32_t)__builtin_clzll(gaps);
        } else {
            // The walk ends: every step takes a 64 lower or stops, and in the word that holds G0 the mask clears the
            // bits below it, so `ones` < 64 there and a stays at or above G0.
            a = wlo;   // (a multiple of 64 while the walk goes on)
            while (a > G0 && b - a + 1 <= k) {
                const uint64_t plo = a - 64;
                unsigned long long pz = ~bits[plo >> 6];
                if (G0 > plo) pz &= ~0ULL << (G0 - plo);
                const uint32_t ones = (pz == ~0ULL) ? 64u : (uint32_t)__builtin_clzll(~pz);
                a -= ones;
                if (ones < 64) break;
            }
        }
        const uint64_t w = b - a + 1;
        const bool head = a == G0, tail = b == G1 - 1;
        if (w > k || w < minw || (head && tail) || (!head && !tail && w != k)) continue;
        const unsigned long long at = atomicAdd(n_sites, 1ULL);
        if (at < site_cap) {
            CorrectSite s;
            s.rec = rec;
            s.a = (uint32_t)(a - G0);
            s.w = (uint32_t)w;
            s.p = tail ? s.a + k - 1 : (uint32_t)(b - G0);
            s.pad = 0;
            sites[at] = s;
        }
    }
}

// The sites of the records [0, min(cap, *d_nrec or nrec)) with line offsets in lo (TL_N words each; the bitmap is
// indexed by the same positions).  A lane takes a record and walks its few words (reads of 100-300 bases are 2-6 words);
// a record of more than CORRECT_LONG_WORDS words is walked by the whole wave, a word per lane.  *n_sites counts every site;
// site_cap is a bound that cannot be exceeded (the host's correct_site_cap).
__global__ __launch_bounds__(NT) void correct_sites_kernel(const unsigned long long *bits, const unsigned long long *lo,
                                                           const unsigned long long *d_nrec, uint64_t nrec, uint64_t cap,
                                                           uint32_t k, uint32_t minw, CorrectSite *sites, uint64_t site_cap,
                                                           unsigned long long *n_sites) {
    const uint64_t R = min(cap, d_nrec ? (uint64_t)*d_nrec : nrec);
    const int lane = threadIdx.x & 63;
    // wave-uniform trip counts: r0 is the same for every lane of a wave
    for (uint64_t r0 = ((uint64_t)blockIdx.x * NT + threadIdx.x) & ~63ULL; r0 < R; r0 += (uint64_t)gridDim.x * NT) {
        const uint64_t r = r0 + lane;
        uint64_t G0 = 0, G1 = 0;
        if (r < R) {
            const uint64_t s2 = lo[r * TL_N + 2], e2 = lo[r * TL_N + 3];
            if (e2 > s2 && e2 - s2 >= (uint64_t)k + 1) { G0 = s2; G1 = e2 - k + 1; }   // n = L - k + 1 >= 2
        }
        const bool has = G1 > G0;
        const uint64_t w0 = G0 >> 6, w1 = has ? (G1 - 1) >> 6 : 0;
        const bool is_long = has && w1 - w0 + 1 > CORRECT_LONG_WORDS;
        if (has && !is_long)
            for (uint64_t wi = w0; wi <= w1; ++wi) correct_word_runs(bits, wi, G0, G1, k, minw, r, sites, site_cap, n_sites);
        for (unsigned long long lm = __ballot(is_long); lm; lm &= lm - 1) {
            const int src = __builtin_ctzll(lm);
            const uint64_t g0 = __shfl((unsigned long long)G0, src, 64), g1 = __shfl((unsigned long long)G1, src, 64);
            for (uint64_t wi = (g0 >> 6) + lane; wi <= ((g1 - 1) >> 6); wi += 64)
                correct_word_runs(bits, wi, g0, g1, k, minw, r0 + src, sites, site_cap, n_sites);
        }
    }
}

// What one wave wrote to LDS is readable by its other lanes (a wave's LDS operations complete in order; this keeps the
// compiler from moving them across).
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

struct CorrectArgs {
    uint64_t lower, upper;   // a window is solid when lower <= count <= upper
    uint64_t rec_base;       // the record number of lo[0] in the text
    uint64_t text_n;         // readable bytes of the text
};

constexpr int CORRECT_STAGE_WORDS = 10;   // 2-bit codes of 256 bases, and two zero words (extract_kmer reads on)

// One site per wave (sites [0, min(*n_sites, site_cap)), waves stride).  The wave stages the w + k - 1 <= 2k - 1 bases its
// windows cover as 2-bit codes in LDS (and, ACGT_ONLY, which of them are outside ACGTacgt); lane i of a round of 64 takes
// window a + i: one hash (two on a canonical table), then per alternative d = 1..3 one XOR with the LUT's entry of the
// suspect base's offset j = p - (a + i) and one probe (first_probe / lookup_rest: the count rule of probe_round_count,
// carried counts included).  An alternative is good when no lane of the site found its window non-solid.  Exactly one
// good alternative: lane 0 appends the correction (corr[at] for at < corr_cap; tot[CT_CORRECTED] counts them all and is
// the append cursor).  The other two totals are summed per wave and added once per workgroup.
// Dynamic LDS: the LUT.
template <int WK, bool CANON, bool ACGT_ONLY>
__global__ __launch_bounds__(NT) void correct_probe_kernel(TableParams p, CorrectArgs ca, const uint8_t *text,
                                                           const unsigned long long *lo, const CorrectSite *sites,
                                                           const unsigned long long *n_sites, uint64_t site_cap,
                                                           CorrectionRec *corr, uint64_t corr_cap, unsigned long long *tot) {
    __shared__ uint64_t s_codes[NT / 64][CORRECT_STAGE_WORDS];
    __shared__ uint8_t s_bad[NT / 64][64], s_badpre[NT / 64][64];
    __shared__ unsigned int s_tot[CT_N];
    extern __shared__ uint64_t s_lut[];

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int lut_words = p.groups * (1 << p.g) * WK;
    for (int i = tid; i < lut_words; i += NT) s_lut[i] = p.lut[i];
    if (tid < CT_N) s_tot[tid] = 0;
    if (lane < 2) s_codes[wv][CORRECT_STAGE_WORDS - 2 + lane] = 0;
    __syncthreads();

    const uint32_t k = (uint32_t)p.k;
    const uint64_t ns = min((uint64_t)*n_sites, site_cap);
    unsigned int n_amb = 0, n_unf = 0;   // (wave-uniform)
    for (uint64_t si = (uint64_t)blockIdx.x * (NT / 64) + wv; si < ns; si += (uint64_t)gridDim.x * (NT / 64)) {
        const CorrectSite s = sites[si];
        const uint64_t s2 = lo[s.rec * TL_N + 2];
        const uint64_t at0 = s2 + s.a;            // the text byte of base 0 of window a
        const uint32_t span = s.w + k - 1;        // bases the windows a .. a + w - 1 cover (<= 253)
        const uint64_t pp = s2 + s.p;
        const uint32_t pb = pp < ca.text_n ? text[pp] : (uint32_t)'\n';
        const uint32_t pl = pb | 0x20u;
        if (!(pl == 'a' || pl == 'c' || pl == 'g' || pl == 't')) { ++n_unf; continue; }   // (wave-uniform)

        // stage: four bases per lane, one byte of codes
        uint32_t code8 = 0, bad4 = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t i = (uint32_t)lane * 4 + q;
            uint32_t b = 'A';
            if (i < span && at0 + i < ca.text_n) b = text[at0 + i];
            code8 |= base_code(b) << (2 * q);
            if constexpr (ACGT_ONLY) {
                const uint32_t l = b | 0x20u;
                bad4 |= (l == 'a' || l == 'c' || l == 'g' || l == 't') ? 0u : (1u << q);
            }
        }
        reinterpret_cast<uint8_t *>(s_codes[wv])[lane] = (uint8_t)code8;
        if constexpr (ACGT_ONLY) {
            const uint32_t c = __popc(bad4);
            s_bad[wv][lane] = (uint8_t)bad4;
            s_badpre[wv][lane] = (uint8_t)(wave_incl_scan(c) - c);   // bad bases in front of the lane's four (<= 252)
        }
        wave_lds_sync();

        unsigned int fail = 0;   // bit d - 1: alternative d met a non-solid window (wave-uniform)
        for (uint32_t i0 = 0; i0 < s.w; i0 += 64) {
            const uint32_t i = i0 + lane;
            const bool act = i < s.w;
            bool f[3] = {false, false, false};
            if (act) {
                bool dropped = false;
                if constexpr (ACGT_ONLY) {
                    // bad bases in [i, i + k): prefix counts at both ends (a lane's four are one nibble)
                    // (i + k <= 253: both ends lie in the stage)
                    auto before = [&](uint32_t e) { return s_badpre[wv][e >> 2] + __popc(s_bad[wv][e >> 2] & ((1u << (e & 3)) - 1u)); };
                    dropped = before(i + k) != before(i);
                }
                if (dropped) {
                    f[0] = f[1] = f[2] = true;
                } else {
                    uint64_t x[WK], h[WK], hr[WK];
                    extract_kmer<WK>(s_codes[wv], i, p.top_mask, x);
                    hash_apply<WK>(p, (const uint64_t *)s_lut, x, h);
                    if constexpr (CANON) {
                        uint64_t rx[WK];
                        revcomp<WK>(x, p.n, rx);
                        hash_apply<WK>(p, (const uint64_t *)s_lut, rx, hr);
                    }
                    const uint32_t j = s.p - s.a - i;            // the suspect base's offset in this window
                    const uint32_t bj = 2 * j, br = 2 * (k - 1 - j);
                    const uint32_t gj = bj / (uint32_t)p.g, gr = br / (uint32_t)p.g;
#pragma unroll
                    for (uint32_t d = 1; d <= 3; ++d) {
                        const uint64_t *ej = s_lut + (size_t)((gj << p.g) + (d << (bj - gj * p.g))) * WK;
                        uint64_t q[WK];
#pragma unroll
                        for (int t = 0; t < WK; ++t) q[t] = h[t] ^ ej[t];
                        if constexpr (CANON) {
                            const uint64_t *er = s_lut + (size_t)((gr << p.g) + (d << (br - gr * p.g))) * WK;
                            uint64_t o[WK];
#pragma unroll
                            for (int t = 0; t < WK; ++t) o[t] = hr[t] ^ er[t];
                            key_min<WK>(q, o);
                        }
                        const uint64_t c = lookup_rest<WK>(p, q, first_probe<WK>(p, q));
                        f[d - 1] = c < ca.lower || c > ca.upper;
                    }
                }
            }
#pragma unroll
            for (int d = 0; d < 3; ++d) fail |= (__ballot(f[d]) != 0ULL) ? (1u << d) : 0u;
        }
        wave_lds_sync();   // the stage is read before the next site overwrites it

        const unsigned int good = ~fail & 7u;
        if (good == 0u) { ++n_unf; continue; }
        if (good & (good - 1u)) { ++n_amb; continue; }
        if (lane == 0) {
            const uint32_t d = (uint32_t)__builtin_ctz(good) + 1u;
            const unsigned long long at = atomicAdd(tot + CT_CORRECTED, 1ULL);
            if (at < corr_cap) {
                CorrectionRec r;
                r.record = ca.rec_base + s.rec;
                r.pos = s.p;
                r.from = (uint8_t)pb;
                r.to = (uint8_t)((uint32_t)"ACGT"[base_code(pb) ^ d] | (pb & 0x20u));
                r.windows = (uint16_t)s.w;
                corr[at] = r;
            }
        }
    }
    if (lane == 0) {
        if (n_amb) atomicAdd(&s_tot[CT_AMBIGUOUS], n_amb);
        if (n_unf) atomicAdd(&s_tot[CT_UNFIXABLE], n_unf);
    }
    __syncthreads();
    if (tid < CT_N && tid != CT_CORRECTED && s_tot[tid]) atomicAdd(tot + tid, (unsigned long long)s_tot[tid]);
}

// out[start of the sequence line of corr[i].record + pos] = to, for the corrections [0, min(*n_corr, corr_cap)) of the
// records from rec_base on (lo[0] is record rec_base).  One lane per correction.  `total` (optional): *total = total_value,
// the size of the output the write-behind stages.
__global__ __launch_bounds__(NT) void correct_apply_kernel(const CorrectionRec *corr, const unsigned long long *n_corr,
                                                           uint64_t corr_cap, const unsigned long long *lo, uint64_t rec_base,
                                                           uint8_t *out, uint64_t out_n, unsigned long long *total,
                                                           uint64_t total_value) {
    if (total && blockIdx.x == 0 && threadIdx.x == 0) *total = total_value;
    const uint64_t nc = min((uint64_t)*n_corr, corr_cap);
    for (uint64_t i = (uint64_t)blockIdx.x * NT + threadIdx.x; i < nc; i += (uint64_t)gridDim.x * NT) {
        const CorrectionRec c = corr[i];
        const uint64_t at = lo[(c.record - rec_base) * TL_N + 2] + c.pos;
        if (at < out_n) out[at] = c.to;
    }
}

}  // namespace tsx
