// tsx_fasta.h -- wrapped (multi-line) FASTA: the sequence lines of a record joined on the device.
//
// One primitive, "unwrap a piece": a piece of wrapped text plus a small device-resident carry from the piece before it
// becomes two-line text (">\n" + sequence + "\n" per record) that the scan kernels of tsx_kernels.h read unchanged.  It is
// stream compaction with three dependencies that cross tiles, all scans of the kind the line pass does:
//   h  is this byte inside a header line?   the last of {'>' at a line start, '\n'} in front of it is the '>'
//   q  has the open record sequence yet?    the last non-newline byte in front of it is a sequence byte
//   o  the output offset                    exclusive sum of the emitted lengths
// A sequence byte with q = 0 in front of it is the first of its record and emits "\n>\n" in front of itself, every other
// sequence byte emits itself, newlines and header bytes emit nothing (header text is dropped: nothing downstream of
// counting reads it).  The output of a piece starts one byte early, so that the leading '\n' of its first separator
// falls off the front.
//
//   fasta_summary_kernel     pass 1 over the text: per tile, what it does to (h, q) and the bytes it emits
//   fasta_chunk_kernel       the summaries of SCAN_CHUNK tiles composed into one
//   fasta_chunk_scan_kernel  the chunks walked from the carried state; writes the piece's prefix (">\n" + carried bases)
//   fasta_tile_scan_kernel   state and output offset at every tile start
//   fasta_emit_kernel        pass 2 over the text: the bytes
//   fasta_finish_kernel      the carry for the next piece, out of the tail of what was written
//   fasta_fill_kernel        '\n' from the end of the output to the end of the scratch (empty lines are dropped downstream)
//
// The carry (FA_CARRY_BYTES, device): word 0 = where the piece ended (0 at a line start, 1 inside a header line, 2 inside
// a sequence line), word 1 = q, word 2 = carried bases, bytes 16.. = the last min(k - 1, bases so far) bases of the open
// record.  A piece that continues a record starts with ">\n" + those bases: every output piece is a two-line text of its
// own, and a k-mer across a seam is counted once, in the later piece (k - 1 bases hold no whole window).
#pragma once
#include "tsx_kernels.h"

namespace tsx {

constexpr int FA_CARRY_BYTES = 16 + 128;
constexpr int FA_INFO_WORDS = 4;      // info of a piece (device): output bytes, h | q << 1 at its end
constexpr uint32_t FA_NOPOS = 0xFFFFFFFFu;   // the output position one in front of the buffer

// bit i = byte i of v equals c
__device__ __forceinline__ uint32_t fa_eq16(const uint4 v, uint32_t c) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    const uint32_t cc = c * 0x01010101u;
    uint32_t m = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t z = w[i] ^ cc;
        const uint32_t nz = ((z & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | z;
        uint32_t u = (~nz & 0x80808080u) >> 7;
        u |= u >> 7;
        m |= ((u | (u >> 14)) & 0xFu) << (4 * i);
    }
    return m;
}

// State after each of 16 positions of a set/clear sequence: position i takes `set` bit i where `ev` bit i is set and the
// state of position i - 1 otherwise (cin in front of position 0).  Doubling steps over 17 bits.
__device__ __forceinline__ uint32_t fa_fill16(uint32_t set, uint32_t ev, uint32_t cin) {
    uint32_t s = ((set & ev) << 1) | (cin & 1u), m = ~(ev << 1) & 0x1FFFEu;
    s |= (s << 1) & m; m &= m << 1;
    s |= (s << 2) & m; m &= m << 2;
    s |= (s << 4) & m; m &= m << 4;
    s |= (s << 8) & m; m &= m << 8;
    s |= (s << 16) & m;
    return (s >> 1) & 0xFFFFu;
}

// The state in front of this lane's 16 positions, over the workgroup's tile: every lane says whether it holds an event
// and the state after its last one; the nearest such lane below wins, then the nearest wave below (through s_w, one word
// per wave: 2 | state, or 0), then tile_in.  any / last: the tile holds an event, and the state after its last one;
// clear: nothing in front of this lane in the tile holds one.  Two barriers.
__device__ __forceinline__ uint32_t fa_lane_carry(bool has, uint32_t last_set, uint32_t tile_in, uint32_t *s_w, bool &any,
                                                  uint32_t &last, bool &clear) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const unsigned long long bh = __ballot(has), bs = __ballot(has && last_set);
    __syncthreads();   // (s_w may still be read from the use before)
    if (lane == 0) s_w[wave] = bh ? (2u | (uint32_t)((bs >> (63 - __clzll((long long)bh))) & 1ULL)) : 0u;
    __syncthreads();
    uint32_t win = tile_in;
    bool wclear = true;
    any = false; last = 0;
    for (uint32_t w = 0; w < NT / 64; ++w) {
        const uint32_t x = s_w[w];
        if (x) { any = true; last = x & 1u; if (w < wave) { win = x & 1u; wclear = false; } }
    }
    const unsigned long long below = bh & ((1ULL << lane) - 1ULL);
    clear = wclear && !below;
    if (!below) return win;
    return (uint32_t)((bs >> (63 - __clzll((long long)below))) & 1ULL);
}

// The front end both passes share: the 16 bytes of this lane of `tile` and, for h = h_in at the tile start,
//   hdr    its non-newline bytes of header lines
//   seq    its non-newline bytes of sequence lines (bytes at or past n are newlines)
//   open   its non-newline bytes in front of the first event of the tile: in hdr iff h_in, else in seq
// line0: offset 0 of the piece is a line start.
__device__ __forceinline__ uint4 fa_classes(const uint8_t *buf, uint64_t n, uint64_t tile, bool line0, uint32_t h_in, uint32_t *s_w,
                                            uint32_t &hdr, uint32_t &seq, uint32_t &open, bool &h_any, uint32_t &h_last) {
    const uint64_t off = tile * TILE + (uint64_t)threadIdx.x * 16;
    const uint4 v = load16(buf, off, n);
    const uint32_t valid = (off + 16 <= n) ? 0xFFFFu : (off >= n ? 0u : ((1u << (uint32_t)(n - off)) - 1u));
    const uint32_t nl = fa_eq16(v, (uint32_t)'\n') & valid;
    const bool pnl = (off == 0) ? line0 : (off - 1 < n && buf[off - 1] == (uint8_t)'\n');
    const uint32_t hs = fa_eq16(v, (uint32_t)'>') & ((nl << 1) | (pnl ? 1u : 0u)) & valid;   // '>' at a line start
    const uint32_t ev = hs | nl;
    bool clear;
    const uint32_t cin = fa_lane_carry(ev != 0, ev ? ((hs >> (31 - __clz((int)ev))) & 1u) : 0u, h_in, s_w, h_any, h_last, clear);
    const uint32_t st = fa_fill16(hs, ev, cin);
    const uint32_t body = ~nl & valid;
    hdr = st & body;
    seq = ~st & body;
    open = clear ? (body & (ev ? ((ev & (0u - ev)) - 1u) : 0xFFFFu)) : 0u;
    return v;
}

// The sequence bytes that start a record, for q = q_in at the tile start.  q_any / q_last as in fa_lane_carry;
// lead (one lane at most): the first non-newline byte of the tile is a sequence byte -- the result holds it iff !q_in.
__device__ __forceinline__ uint32_t fa_firsts(uint32_t hdr, uint32_t seq, uint32_t q_in, uint32_t *s_w, bool &q_any, uint32_t &q_last,
                                              bool &lead) {
    const uint32_t ev = hdr | seq;
    bool clear;
    const uint32_t cin = fa_lane_carry(ev != 0, ev ? ((seq >> (31 - __clz((int)ev))) & 1u) : 0u, q_in, s_w, q_any, q_last, clear);
    const uint32_t after = fa_fill16(seq, ev, cin);
    const uint32_t before = ((after << 1) | cin) & 0xFFFFu;
    lead = clear && (seq & ev & (0u - ev)) != 0;
    return seq & ~before;
}

// Tile summary: x, y = bytes emitted for h_in = 0, 1, both with q_in = 1; z = flags.  State s = h | q << 1.
constexpr uint32_t FA_F_EV = 1;      // the tile holds an '>' at a line start or a newline: h_out = FA_F_H, else h_in
constexpr uint32_t FA_F_H = 2;
constexpr uint32_t FA_F_BODY = 4;    // it holds a non-newline byte: q_out = FA_F_Q0 << h_in, else q_in
constexpr uint32_t FA_F_Q0 = 8;
constexpr uint32_t FA_F_LEAD0 = 32;  // (<< h_in) its first non-newline byte is a sequence byte: 3 more bytes when q_in = 0

__device__ __forceinline__ uint32_t fa_next(const uint4 t, uint32_t s) {
    const uint32_t h = s & 1u, q = s >> 1;
    const uint32_t h2 = (t.z & FA_F_EV) ? ((t.z & FA_F_H) ? 1u : 0u) : h;
    const uint32_t q2 = (t.z & FA_F_BODY) ? ((t.z & (FA_F_Q0 << h)) ? 1u : 0u) : q;
    return h2 | (q2 << 1);
}
__device__ __forceinline__ uint32_t fa_emitted(const uint4 t, uint32_t s) {
    const uint32_t h = s & 1u, q = s >> 1;
    return (h ? t.y : t.x) + ((!q && (t.z & (FA_F_LEAD0 << h))) ? 3u : 0u);
}

// Sum over the workgroup (NT threads).  Two barriers.
__device__ __forceinline__ uint32_t fa_block_sum(uint32_t c, uint32_t *s_w) {
    for (int d = 32; d > 0; d >>= 1) c += __shfl_down(c, d, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = c;
    __syncthreads();
    return s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// Pass 1.  The header scan runs once (for h_in = 0: with h_in = 1 only the `open` bytes change sides), the record scan
// once per h_in.
__global__ __launch_bounds__(NT) void fasta_summary_kernel(const uint8_t *buf, uint64_t n, const uint32_t *carry, uint4 *summ,
                                                           uint64_t ntiles) {
    __shared__ uint32_t s_w[NT / 64];
    __shared__ uint32_t s_lead[2];
    const bool line0 = carry[0] == 0u;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        if (threadIdx.x < 2) s_lead[threadIdx.x] = 0;
        uint32_t hdr, seq, open, h_last;
        bool h_any;
        fa_classes(buf, n, tile, line0, 0u, s_w, hdr, seq, open, h_any, h_last);
        uint32_t flags = h_any ? (FA_F_EV | (h_last ? FA_F_H : 0u)) : 0u, cnt[2];
#pragma unroll
        for (uint32_t h = 0; h < 2; ++h) {
            const uint32_t hd = h ? (hdr | open) : hdr, sq = h ? (seq & ~open) : seq;
            uint32_t q_last;
            bool q_any, lead;
            const uint32_t first = fa_firsts(hd, sq, 1u, s_w, q_any, q_last, lead);
            if (lead) s_lead[h] = 1;
            cnt[h] = fa_block_sum(__popc(sq) + 3u * __popc(first), s_w);   // (its barriers publish s_lead)
            if (q_any) flags |= FA_F_BODY | (q_last ? (FA_F_Q0 << h) : 0u);
            if (s_lead[h]) flags |= FA_F_LEAD0 << h;
        }
        if (threadIdx.x == 0) summ[tile] = make_uint4(cnt[0], cnt[1], flags, 0u);
        __syncthreads();   // (s_lead is cleared for the next tile)
    }
}

// What a run of tiles does to each of the four states: out = the state after it (2 bits per state in front),
// e[s] = the bytes it emits.
struct FaFn { uint32_t out; uint32_t e[4]; };
__device__ __forceinline__ FaFn fa_fn_of(const uint4 t) {
    FaFn f; f.out = 0;
#pragma unroll
    for (uint32_t s = 0; s < 4; ++s) { f.out |= fa_next(t, s) << (2 * s); f.e[s] = fa_emitted(t, s); }
    return f;
}
__device__ __forceinline__ uint32_t fa_out_then(uint32_t a, uint32_t b) {   // first a, then b
    uint32_t r = 0;
#pragma unroll
    for (uint32_t s = 0; s < 4; ++s) r |= ((b >> (2 * ((a >> (2 * s)) & 3u))) & 3u) << (2 * s);
    return r;
}
__device__ __forceinline__ FaFn fa_then(const FaFn &a, const FaFn &b) {
    FaFn r; r.out = fa_out_then(a.out, b.out);
#pragma unroll
    for (uint32_t s = 0; s < 4; ++s) {
        const uint32_t mid = (a.out >> (2 * s)) & 3u;
        r.e[s] = a.e[s] + (mid == 0 ? b.e[0] : mid == 1 ? b.e[1] : mid == 2 ? b.e[2] : b.e[3]);
    }
    return r;
}
constexpr uint32_t FA_ID = 0xE4u;   // the identity: state s stays s
constexpr int FA_CHUNK_WORDS = 8;   // a chunk's FaFn in global memory (5 used)

__global__ __launch_bounds__(SCAN_CHUNK) void fasta_chunk_kernel(const uint4 *summ, uint64_t ntiles, uint32_t *chunk_fn) {
    __shared__ FaFn s_f[SCAN_CHUNK / 64];
    const uint64_t i = (uint64_t)blockIdx.x * SCAN_CHUNK + threadIdx.x;
    FaFn f = fa_fn_of(i < ntiles ? summ[i] : make_uint4(0, 0, 0, 0));
    for (int d = 1; d < 64; d <<= 1) {   // lane i (a multiple of 2d) takes [i + d, i + 2d) behind its own [i, i + d)
        FaFn o;
        o.out = __shfl_down(f.out, d, 64);
#pragma unroll
        for (int s = 0; s < 4; ++s) o.e[s] = __shfl_down(f.e[s], d, 64);
        f = fa_then(f, o);
    }
    if ((threadIdx.x & 63) == 0) s_f[threadIdx.x >> 6] = f;
    __syncthreads();
    if (threadIdx.x == 0) {
        FaFn t = s_f[0];
        for (int w = 1; w < SCAN_CHUNK / 64; ++w) t = fa_then(t, s_f[w]);
        uint32_t *o = chunk_fn + (size_t)blockIdx.x * FA_CHUNK_WORDS;
        o[0] = t.out; o[1] = t.e[0]; o[2] = t.e[1]; o[3] = t.e[2]; o[4] = t.e[3];
    }
}

// One workgroup.  chunk_in[2c] = state at the start of chunk c, chunk_in[2c + 1] = output position there; info[0] = bytes
// of output, info[1] = state at the end.  A piece that continues a record with sequence starts with ">\n" + the carried
// bases, any other one byte in front of the buffer (FA_NOPOS).
__global__ __launch_bounds__(NT) void fasta_chunk_scan_kernel(const uint32_t *chunk_fn, uint32_t nchunks, const uint32_t *carry,
                                                              uint32_t kminus1, uint32_t *chunk_in, uint32_t *info, uint8_t *out,
                                                              uint32_t out_cap) {
    const uint32_t q = carry[1] ? 1u : 0u, nb = q ? min(carry[2], kminus1) : 0u;
    if (q) {
        const uint8_t *cb = reinterpret_cast<const uint8_t *>(carry) + 16;
        for (uint32_t i = threadIdx.x; i < 2 + nb; i += NT)
            if (i < out_cap) out[i] = i == 0 ? (uint8_t)'>' : i == 1 ? (uint8_t)'\n' : cb[i - 2];
    }
    if (threadIdx.x == 0) {
        uint32_t s = (carry[0] == 1u ? 1u : 0u) | (q << 1), pos = q ? 2u + nb : FA_NOPOS;
        for (uint32_t c = 0; c < nchunks; ++c) {
            const uint32_t *f = chunk_fn + (size_t)c * FA_CHUNK_WORDS;
            chunk_in[2 * c] = s; chunk_in[2 * c + 1] = pos;
            pos += f[1 + s];
            s = (f[0] >> (2 * s)) & 3u;
        }
        info[0] = pos == FA_NOPOS ? 0u : pos;
        info[1] = s;
    }
}

__global__ __launch_bounds__(SCAN_CHUNK) void fasta_tile_scan_kernel(const uint4 *summ, uint64_t ntiles, const uint32_t *chunk_in,
                                                                     uint32_t *tile_state, uint32_t *tile_pos) {
    __shared__ uint32_t s_f[SCAN_CHUNK / 64], s_c[SCAN_CHUNK / 64];
    const uint64_t i = (uint64_t)blockIdx.x * SCAN_CHUNK + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint4 t = i < ntiles ? summ[i] : make_uint4(0, 0, 0, 0);
    uint32_t f = 0;
#pragma unroll
    for (uint32_t s = 0; s < 4; ++s) f |= fa_next(t, s) << (2 * s);
    for (int d = 1; d < 64; d <<= 1) {   // inclusive scan under composition
        const uint32_t o = __shfl_up(f, d, 64);
        if (lane >= (uint32_t)d) f = fa_out_then(o, f);
    }
    if (lane == 63) s_f[wave] = f;
    __syncthreads();
    uint32_t wf = FA_ID;
    for (uint32_t w = 0; w < wave; ++w) wf = fa_out_then(wf, s_f[w]);
    const uint32_t s0 = chunk_in[2 * blockIdx.x];
    uint32_t excl = __shfl_up(f, 1, 64);
    excl = lane ? fa_out_then(wf, excl) : wf;
    const uint32_t s_in = (excl >> (2 * s0)) & 3u;
    const uint32_t e = fa_emitted(t, s_in), inc = wave_incl_scan(e);
    if (lane == 63) s_c[wave] = inc;
    __syncthreads();
    uint32_t pos = chunk_in[2 * blockIdx.x + 1] + inc - e;
    for (uint32_t w = 0; w < wave; ++w) pos += s_c[w];
    if (i < ntiles) { tile_state[i] = s_in; tile_pos[i] = pos; }
}

// Pass 2.
__global__ __launch_bounds__(NT) void fasta_emit_kernel(const uint8_t *buf, uint64_t n, const uint32_t *carry, const uint32_t *tile_state,
                                                        const uint32_t *tile_pos, uint64_t ntiles, uint8_t *out, uint32_t out_cap) {
    __shared__ uint32_t s_w[NT / 64];
    const bool line0 = carry[0] == 0u;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint32_t s = tile_state[tile];
        uint32_t hdr, seq, open, h_last, q_last;
        bool h_any, q_any, lead;
        const uint4 v = fa_classes(buf, n, tile, line0, s & 1u, s_w, hdr, seq, open, h_any, h_last);
        const uint32_t first = fa_firsts(hdr, seq, s >> 1, s_w, q_any, q_last, lead);
        const uint32_t c = __popc(seq) + 3u * __popc(first), inc = wave_incl_scan(c);
        __syncthreads();
        if ((threadIdx.x & 63) == 63) s_w[threadIdx.x >> 6] = inc;
        __syncthreads();
        uint32_t pos = tile_pos[tile] + inc - c;
        for (uint32_t w = 0; w < (threadIdx.x >> 6); ++w) pos += s_w[w];
        const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (uint32_t i = 0; i < 16; ++i) {
            if (!((seq >> i) & 1u)) continue;
            if ((first >> i) & 1u) {   // (FA_NOPOS: the separator's newline in front of the whole output)
                if (pos < out_cap) out[pos] = (uint8_t)'\n';
                if (pos + 1 < out_cap) out[pos + 1] = (uint8_t)'>';
                if (pos + 2 < out_cap) out[pos + 2] = (uint8_t)'\n';
                pos += 3;
            }
            if (pos < out_cap) out[pos] = (uint8_t)(w4[i >> 2] >> (8 * (i & 3)));
            ++pos;
        }
    }
}

// One workgroup of 128 threads: the carry after this piece.  The open record's bases are the last line of the output
// (which holds the bases carried in, when the record came from the piece before): its last min(k - 1, length) bytes.
__global__ __launch_bounds__(128) void fasta_finish_kernel(const uint8_t *buf, uint64_t n, const uint32_t *info, const uint8_t *out,
                                                           uint32_t kminus1, uint32_t *carry) {
    __shared__ uint8_t s_b[128];
    __shared__ uint32_t s_src, s_nb;
    const uint32_t total = info[0], s = info[1], q = s >> 1;
    const uint32_t ws = total > 128u ? total - 128u : 0u, wn = total - ws;
    s_b[threadIdx.x] = (q && threadIdx.x < wn) ? out[ws + threadIdx.x] : (uint8_t)0;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t start = 0;
        for (uint32_t i = 0; i < wn; ++i) if (s_b[i] == (uint8_t)'\n') start = i + 1;
        const uint32_t nb = q ? min(wn - start, kminus1) : 0u;
        s_nb = nb; s_src = wn - nb;
    }
    __syncthreads();
    uint8_t *cb = reinterpret_cast<uint8_t *>(carry) + 16;
    if (threadIdx.x < s_nb) cb[threadIdx.x] = s_b[s_src + threadIdx.x];
    if (threadIdx.x == 0) {
        if (n) carry[0] = buf[n - 1] == (uint8_t)'\n' ? 0u : ((s & 1u) ? 1u : 2u);
        carry[1] = q;
        carry[2] = s_nb;
    }
}

// out[info[0], end) = '\n', 16 bytes per thread.
__global__ __launch_bounds__(NT) void fasta_fill_kernel(const uint32_t *info, uint8_t *out, uint64_t end) {
    const uint64_t from = info[0];
    const uint64_t b0 = from / 16, b1 = (end + 15) / 16;
    for (uint64_t b = b0 + (uint64_t)blockIdx.x * NT + threadIdx.x; b < b1; b += (uint64_t)gridDim.x * NT) {
        const uint64_t lo = b * 16, hi = lo + 16;
        if (lo >= from && hi <= end) {
            *reinterpret_cast<uint4 *>(out + lo) = make_uint4(0x0A0A0A0Au, 0x0A0A0A0Au, 0x0A0A0A0Au, 0x0A0A0A0Au);
        } else {
            for (uint64_t p = lo > from ? lo : from; p < hi && p < end; ++p) out[p] = (uint8_t)'\n';
        }
    }
}

}  // namespace tsx
