// tsxcount_hip.hip -- C ABI (include/tsxcount_hip.h) over the HIP kernels.
// Host side only: layout derivation, the bijective mapping and its lookup
// tables, launches, staging copies.  No CPU counting path exists here.
#include "../../include/tsxcount_hip.h"
#include "tsx_kernels.h"
#include "tsx_partition.h"
#include "tsx_minimizer.h"
#include "tsx_inflate.h"
#include "tsx_output.h"
#include "tsx_query.h"
#include "tsx_baserule.h"
#include "tsx_db.h"
#include "tsx_combine.h"
#include "tsx_joint.h"
#include "tsx_het.h"
#include "tsx_unitig.h"
#include "tsx_bin.h"
#include "tsx_fasta.h"
#include "tsx_seq.h"
#include "tsx_track.h"
#include "tsx_trim.h"
#include "tsx_correct.h"
#include "tsx_normalize.h"
#include "tsx_sketch.h"
#include "tsx_prefilter.h"
#include "tsx_pairs.h"
#include "tsx_own.h"

#include <mutex>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cerrno>
#include <chrono>
#include <cmath>
#include <cstring>
#include <deque>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include <unistd.h>

using namespace tsx;

static thread_local std::string g_last_error;

#define HIP_TRY(expr)                                                                    \
    do {                                                                                 \
        hipError_t _e = (expr);                                                          \
        if (_e != hipSuccess) {                                                          \
            g_last_error = std::string(#expr) + ": " + hipGetErrorString(_e);            \
            return (_e == hipErrorOutOfMemory) ? TSX_HIP_ENOMEM : TSX_HIP_EHIP;          \
        }                                                                                \
    } while (0)
// the same for a step that returns a TSX_HIP_* code (the owners' alloc / reserve / create among them)
#define TSX_TRY(expr)                                                                    \
    do {                                                                                 \
        const int _rc = (expr);                                                          \
        if (_rc != TSX_HIP_OK) return _rc;                                               \
    } while (0)

int tsx::own_fail(const char *what, hipError_t e) {
    g_last_error = std::string(what) + ": " + hipGetErrorString(e);
    return (e == hipErrorOutOfMemory) ? TSX_HIP_ENOMEM : TSX_HIP_EHIP;
}

static const int SCAN_WG_PER_CU = 5;  // walk_log_kernel workgroups per CU
static const uint32_t OVQ_CAP = 2048;  // keys per overflow queue (one queue per level-2 workgroup: 32 MiB at 2048 workgroups)
static const size_t STAGE_PIECE_DEFAULT = (size_t)64 << 20;  // bytes of FASTQ per host piece

struct PartPlan {
    int g;                       // regions of the key log (= scan waves, or cuts of a received array)
    int rw;                      // 64-bit words per record
    uint64_t log_cap;            // records per log region
    int b1, b2;                  // radix bits of level 1 / level 2 (b2 == 0: one level)
    uint32_t nb1, nb2, nseg, cpr2;
    uint64_t cap_sub;            // records per level-2 sub-list
    uint32_t hist_nb;            // bins of the scan-side histogram (nb1, or #owners for a sharded scan)
    unsigned long long *c_log, *c_rstart, *c_bstart, *c_bcnt, *c_seg, *d_offs;
    uint32_t *d_hist;
    size_t cnt_need;
    // walk fused with level 1 (walk_part_kernel): G1 workgroups, each with a sub-list of cap1 records per level-1
    // bucket in buffer 1: list (b, g) at number * cap1, its size in c_l1[number], the number by tsx_layout.h --
    // b * G1 + g, or g * nb1 + b (l1_wgm) once the LOCAL walk of a plain one-GPU count has filled them
    bool fused;
    bool l1_wgm;
    uint32_t G1;
    uint64_t cap1;
    unsigned long long *c_l1;
    uint64_t *buf1;              // buffer 1 of this plan (the map's, or the window-wise sharded level 1's own)
};

// What the last fused walk of a plain count left (tsx_hip_level1_sizes_host): where its list sizes lie in d_cnt, and the
// shape and order of the lists.
struct L1Seen { size_t at = 0; uint32_t nb = 0, G = 0, cpr2 = 0; uint64_t cap = 0; int wg_major = 0; };

// Ownership (tsx_own.h): every device buffer, pinned buffer, event and stream of a map is a member that releases
// itself -- adding one is adding a member, nothing else.  The capacities are the owners' (bytes).  TableParams only
// borrows: it goes to the kernels by value, so `p` holds copies of get().
struct tsx_hip_map {
    TableParams p{};
    tsx_hip_layout lay{};
    int device = 0;
    uint64_t seed = 0;
    Stream stream;                       // declared in front of every buffer: it outlives them
    Stream copy_stream;                  // H2D copies of the host entry point
    // bijective mapping, host copy: rows[i] yields output bit n-1-i
    std::vector<uint64_t> rows, irows;   // n x wk
    std::vector<uint64_t> lut, ilut;     // [groups][1<<g][wk]
    DevBuf<uint64_t> table, sec_keys, sec_cnt;   // what p.table, p.sec_keys, p.sec_cnt, p.stats, p.seg_dirty, p.lut,
    DevBuf<unsigned long long> stats;            // p.ilut and p.roll point to
    DevBuf<uint8_t> seg_dirty;
    DevBuf<uint64_t> d_lut, d_ilut, d_roll;
    DevBuf<uint64_t> d_ovq;              // overflow queues of the level-2 partition (OVQ_CAP records per workgroup)
    DevBuf<uint64_t> d_def_rec, d_def_cnt;   // deferred list (DeferList, tsx_device.h)
    DevBuf<unsigned long long> d_def_n;
    uint64_t def_cap() const { return d_def_cnt.cap() / 8; }   // its records
    DeferList defer() const { return DeferList{d_def_rec.get(), d_def_cnt.get(), d_def_n.get(), def_cap()}; }
    bool fresh = false;                  // tsx_hip_clear() was called and the table itself has not been zeroed yet:
                                         // the next partitioned build writes every segment, anything else zeroes first
    DevBuf<uint32_t> d_ovq_cnt;
    uint64_t roll[64] = {0};             // one-limb keys: sliding-window hash update table
    std::vector<uint64_t> roll_wide;     // multi-limb keys: the same, key_limbs words per entry
    uint64_t mroll[64] = {0};            // the mirror roll of the reverse complement's hash (canonical walks)
    std::vector<uint64_t> mroll_wide;
    bool canon = false;                  // canonical counting (tsx_hip_set_canonical)
    uint32_t minq = 0;                   // base rule (tsx_hip_set_base_rule): min_qual_char, 0 = off; acgt_only is p.acgt_only
    DevBuf<uint16_t> d_qmap;             // its low-quality bitmap (tsx_baserule.h)
    const uint16_t *qmap_cur = nullptr;  // the bitmap at the text the next scan launches read (set per call, else null)
    DevBuf<unsigned long long> d_qrec;   // line spans per record behind it, and record cuts
    bool used = false;                   // something was inserted since the map was created or cleared
    // read correction (tsx_correct.h): grow-only scratch, kept between calls
    struct CorrectScratch {
        DevBuf<unsigned long long> bits, lo, nsites, tot;   // bitmap, line offsets, the site cursor, a device call's totals
        DevBuf<CorrectSite> sites;
        DevBuf<CorrectionRec> corr;
    } correct;
    // FASTQ scratch
    DevBuf<uint32_t> d_tile;             // tile counts, then one partial sum per SCAN_CHUNK tiles
    uint64_t tile_cap = 0;               // tiles it has room for: where the partial sums start (ensure_tiles)
    DevBuf<uint32_t> d_carry;
    DevBuf<unsigned long long> d_seg;    // 64 owner counters / cursors
    // host staging
    PinBuf<uint8_t> h_stage[2];
    DevBuf<uint8_t> d_stage[2];
    Event stage_done[2];                 // kernels that read d_stage[i] have finished
    Event stage_in[2];                   // the H2D copy into d_stage[i] has finished
    size_t piece = STAGE_PIECE_DEFAULT;  // TSX_HIP_PIECE_BYTES overrides (tests exercise piece seams)
    bool piece_fixed = false;
    int cus = 256;
    // partitioned insert path (tsx_partition.h): grow-only scratch
    int path = 0;                    // 0 auto, 1 atomic, 2 partitioned (tsx_hip_set_path / TSX_HIP_PATH)
    DevBuf<uint64_t> d_buf[2];
    DevBuf<unsigned long long> d_cnt;      // [log regions | level-1 lists | segment lists]
    L1Seen l1_seen;
    // optional per-pass timing (HIP events on the launch stream)
    DevBuf<uint64_t> d_small;        // scratch of tsx_hip_get_counts_host / tsx_hip_lookup_host for a few k-mers
    bool attr_done = false;          // dynamic-LDS limits of the partition / build kernels set on this map's device
    int timing = 0;
    std::vector<Event> ev;           // eight per piece: before pass 1, before pass 3, after pass 3, start of the
                                     // partition phase (later than the scan's end only in a sharded run: the
                                     // exchange lies between), after level 1, level 2, build, the inserts behind it
    std::vector<unsigned long long> h_regions;   // host copy of the region table of a sharded build (starts, then sizes)
    std::unique_ptr<PartPlan> sh_pl;             // sharded run, level 1 per exchange window: the plan made at window 0,
    uint32_t sh_rw = 0, sh_windows = 0;          // regions per window, windows of the step,
    uint32_t mz_regions = 0; uint64_t mz_dcap = 0; size_t mz_len = 0;   // minimizer exchange: the described text waiting in buffer 1 (regions x capacity; its bytes)
    bool sh_ev3 = false;                         // stage timing: the walks of a description exchange have recorded event 3
    DevBuf<unsigned long long> d_desc_cnt;       // strips described per wave of strip_desc_kernel (key log form)
    DevBuf<uint64_t> sh_buf1;                    // and its own sub-list buffer and counters (the scans of the later
    DevBuf<unsigned long long> sh_cnt;           // windows plan with -- and clear -- the map's while level 1 of the
                                                 // earlier ones has already left its sizes there)
    std::deque<long> ev_open;        // tuples of shard scans whose partition phase has not run yet (oldest first)
    size_t ev_used = 0;
    // Ordering between the map's own stream and a caller's stream (the `stream` argument of the *_device entry
    // points): tsx_hip_clear works on the map's stream and records clear_ev behind it; every entry point that
    // launches on a caller's stream waits for that event first.  The other way round, the last caller's stream
    // is remembered (`foreign`) and tsx_hip_clear / tsx_hip_sync order themselves behind what was queued there.
    DevBuf<uint8_t> d_slabdesc;         // count_slabs: the descriptions of every text window, then one counter per window
    // wrapped FASTA (tsx_fasta.h): the two-line text of one piece, the scan scratch, the carry between pieces
    DevBuf<uint8_t> d_fa_out;
    DevBuf<uint32_t> d_fa_ws;
    DevBuf<uint32_t> d_fa_carry;
    // prefilter (tsx_prefilter.h): filter A of 2^pf_bits bits, B of a quarter, the totals (PfTotal); pf_bits 0 = none
    DevBuf<unsigned long long> pf_a, pf_b, pf_tot;
    int pf_bits = 0;
    bool pf_armed = false;               // the FASTQ counting calls consult B (tsx_hip_prefilter_arm)
    Event pf_ev;                         // what the map's stream holds for the filters, for a caller's stream to wait for
    PfView pf_view() const { return PfView{pf_b.get(), pf_tot.get() + PF_ADMITTED, pf_tot.get() + PF_SKIPPED, pf_bits}; }
    uint64_t norm_tiles = 0, norm_skipped = 0;   // the last normalization: tiles its count launches covered, tiles the gate skipped
    Event clear_ev, join_ev;
    bool clear_ev_set = false;
    hipStream_t foreign = nullptr;       // (a caller's: not owned)
    // A map without a stream never touched the device (db_source_params builds one for its host fields).
    ~tsx_hip_map() {
        if (!stream.get()) return;
        (void)hipSetDevice(device);
        (void)hipStreamSynchronize(stream.get());
    }
};

static const size_t STAGE_PAD = 256;
// The timing events of one tuple (a piece, a window, a slab), in stream order: before the line pass, before the scan or
// the description, after it, start of the partition phase (later than the scan's end only in a sharded run: the exchange
// lies between), after level 1, after level 2, after the build kernel, after the inserts behind it.
enum TimingEvent { EV_BEGIN = 0, EV_SCAN, EV_SCAN_END, EV_PART, EV_L1_END, EV_L2_END, EV_BUILD_END, EV_END, EV_N };
static bool can_partition(const tsx_hip_map *m);
static int clear_impl(tsx_hip_map *m, bool full);
static int ensure_zeroed(tsx_hip_map *m, hipStream_t st);
static inline void join_foreign(tsx_hip_map *m, bool host_wait);

extern "C" int tsx_hip_key_limbs(int k) { return (k < 1 || k > 127) ? TSX_HIP_EINVAL : (2 * k + 63) / 64; }

extern "C" const char *tsx_hip_strerror(int code) {
    switch (code) {
        case TSX_HIP_OK: return "ok";
        case TSX_HIP_EINVAL: return "Invalid lengths for hashmap size and value of k";
        case TSX_HIP_ENODEVICE: return "no HIP device";
        case TSX_HIP_ENOMEM: return "device memory exhausted";
        case TSX_HIP_EHIP: return "HIP runtime error";
        case TSX_HIP_EFULL: return "Could not insert kmer: table full";
        case TSX_HIP_EOVERFLOW: return "count overflow array full";
        case TSX_HIP_ERANGE: return "output buffer too small";
        case TSX_HIP_ELOCK: return "a multi-limb slot stayed locked past the spin bound";
        case TSX_HIP_EIO: return "writing the output failed";
        case TSX_HIP_EFORMAT: return "not a k-mer database, or a damaged one";
        case TSX_HIP_EPAIR: return "the mates of a pair do not line up";
    }
    return "unknown";
}
extern "C" const char *tsx_hip_last_error(void) { return g_last_error.c_str(); }

extern "C" int tsx_hip_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

static inline unsigned code_of(unsigned char b) { return ((b >> 1) ^ (b >> 2)) & 3u; }

extern "C" int tsx_hip_encode(const char *seq, int k, uint64_t *out) {
    if (!seq || !out || k < 1 || k > 127) return TSX_HIP_EINVAL;
    const int wk = (2 * k + 63) / 64;
    memset(out, 0, (size_t)wk * 8);
    for (int i = 0; i < k; ++i) out[(2 * i) >> 6] |= (uint64_t)code_of((unsigned char)seq[i]) << ((2 * i) & 63);
    return TSX_HIP_OK;
}
extern "C" int tsx_hip_decode(const uint64_t *limbs, int k, char *out) {
    if (!limbs || !out || k < 1 || k > 127) return TSX_HIP_EINVAL;
    for (int i = 0; i < k; ++i) out[i] = "ACGT"[(limbs[(2 * i) >> 6] >> ((2 * i) & 63)) & 3];
    out[k] = 0;
    return TSX_HIP_OK;
}

// ---- bijective GF(2) mapping ------------------------------------------------
// The reference draws a random UNIT UPPER TRIANGULAR matrix over GF(2)
// (BijectiveKMapping::getRandomMatrix, BijectiveKMapping.h:284-303; row i carries bit
// n-1-j = M[i][j] (matrixToRows, :227-256) and yields output bit n-1-i (applyto,
// :202-225)).  With that family output bit p depends only on input bits <= p, so the
// slot index (the low l bits) is a function of the first l/2 bases alone: all k-mers
// that share a 15-base prefix share one home slot AND one probe sequence.  The
// reference survives that with up to 2^l reprobes; an 8-bit reprobe field does not
// (AT-rich reads at load 0.48 already exhausted 255 probes, scripts/skew_check.py).
// So the matrix here is not triangular (make_mapping() below: multiplication by a random
// field element for one-limb keys, L * U for longer ones): still bijective and
// GF(2)-linear (same IBijectiveFunction contract, same LUT evaluation), but every
// key bit reaches the slot index.  Counts do not depend on the matrix.  Seeded
// splitmix64 replaces srand(time(NULL)).
static uint64_t splitmix_next(uint64_t &st) {
    uint64_t z = (st += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
static inline int rbit(const uint64_t *r, int i) { return (int)((r[i >> 6] >> (i & 63)) & 1); }
static inline void rset(uint64_t *r, int i) { r[i >> 6] |= 1ULL << (i & 63); }

// Irreducible polynomials over GF(2) of degree 2, 4, ..., 64 (low terms; the leading term is
// implied): trinomials where one exists, else pentanomials.  Found with Rabin's test; a wrong
// entry would make the one-limb mapping singular, which make_mapping() reports.
static const uint64_t GF_POLY_LOW[33] = {0, 0x3ULL, 0x3ULL, 0x3ULL, 0x87ULL, 0x9ULL, 0x9ULL, 0x21ULL, 0x47ULL, 0x9ULL, 0x9ULL,
    0x3ULL, 0x87ULL, 0x47ULL, 0x3ULL, 0x3ULL, 0x813ULL, 0x81ULL, 0x201ULL, 0x87ULL, 0x20BULL, 0x81ULL, 0x21ULL, 0x3ULL,
    0x823ULL, 0x207ULL, 0x9ULL, 0x201ULL, 0x8403ULL, 0x80001ULL, 0x3ULL, 0x20000001ULL, 0x807ULL};

static inline uint64_t gf_mulz(uint64_t a, uint64_t plow, int n) {  // a * z in GF(2^n)
    const uint64_t top = (a >> (n - 1)) & 1ULL;
    a <<= 1;
    if (n < 64) a &= (1ULL << n) - 1ULL;
    return top ? (a ^ plow) : a;
}
static inline uint64_t gf_mul(uint64_t a, uint64_t b, uint64_t plow, int n) {
    uint64_t r = 0;
    for (int i = 0; i < n; ++i) {
        if ((b >> i) & 1ULL) r ^= a;
        a = gf_mulz(a, plow, n);
    }
    return r;
}

// Degrees 66..254 (multi-limb keys): x^n + x^a [+ x^b + x^c] + 1, found by scripts/find_irreducible.py
// (Rabin's test); the rows for degrees <= 64 are not used (GF_POLY_LOW above keeps the one-limb mapping
// what it was).  A wrong entry would make the mapping singular, which make_mapping() reports.
static const uint8_t GF_POLY_EXP[127][3] = {  // degree 2, 4, ..., 254: x^n + x^a [+ x^b + x^c] + 1
    {1, 0, 0}, {1, 0, 0}, {1, 0, 0}, {4, 3, 1}, {3, 0, 0}, {3, 0, 0}, {5, 0, 0}, {5, 3, 1},
    {3, 0, 0}, {3, 0, 0}, {1, 0, 0}, {4, 3, 1}, {4, 3, 1}, {1, 0, 0}, {1, 0, 0}, {7, 3, 2},
    {7, 0, 0}, {9, 0, 0}, {6, 5, 1}, {5, 4, 3}, {7, 0, 0}, {5, 0, 0}, {1, 0, 0}, {5, 3, 2},
    {4, 3, 2}, {3, 0, 0}, {9, 0, 0}, {7, 4, 2}, {19, 0, 0}, {1, 0, 0}, {29, 0, 0}, {4, 3, 1},
    {3, 0, 0}, {9, 0, 0}, {5, 3, 1}, {10, 9, 3}, {35, 0, 0}, {21, 0, 0}, {6, 5, 3}, {9, 4, 2},
    {8, 3, 1}, {5, 0, 0}, {21, 0, 0}, {7, 6, 2}, {27, 0, 0}, {21, 0, 0}, {21, 0, 0}, {10, 9, 6},
    {11, 0, 0}, {15, 0, 0}, {29, 0, 0}, {4, 3, 1}, {15, 0, 0}, {17, 0, 0}, {33, 0, 0}, {5, 4, 3},
    {5, 3, 2}, {4, 2, 1}, {33, 0, 0}, {4, 3, 1}, {6, 2, 1}, {19, 0, 0}, {21, 0, 0}, {7, 2, 1},
    {3, 0, 0}, {17, 0, 0}, {57, 0, 0}, {5, 3, 2}, {8, 7, 1}, {15, 0, 0}, {21, 0, 0}, {7, 4, 2},
    {71, 0, 0}, {27, 0, 0}, {53, 0, 0}, {6, 3, 2}, {15, 0, 0}, {9, 0, 0}, {8, 6, 5}, {5, 3, 2},
    {27, 0, 0}, {10, 8, 7}, {37, 0, 0}, {15, 3, 2}, {11, 0, 0}, {1, 0, 0}, {13, 0, 0}, {11, 3, 2},
    {31, 0, 0}, {3, 0, 0}, {81, 0, 0}, {9, 8, 7}, {11, 0, 0}, {6, 5, 2}, {8, 7, 6}, {7, 2, 1},
    {87, 0, 0}, {3, 0, 0}, {9, 0, 0}, {5, 3, 2}, {55, 0, 0}, {27, 0, 0}, {10, 9, 5}, {9, 3, 1},
    {7, 0, 0}, {105, 0, 0}, {73, 0, 0}, {7, 3, 1}, {11, 0, 0}, {7, 0, 0}, {5, 4, 2}, {9, 8, 3},
    {10, 7, 3}, {113, 0, 0}, {8, 7, 6}, {9, 4, 2}, {31, 0, 0}, {5, 0, 0}, {73, 0, 0}, {8, 5, 3},
    {95, 0, 0}, {111, 0, 0}, {11, 2, 1}, {15, 14, 10}, {103, 0, 0}, {15, 0, 0}, {7, 2, 1},
};

struct Big { uint64_t w[4]; };   // an element of GF(2^n), n <= 254: bit i of the polynomial in w[i / 64]
static inline Big big_zero() { Big b; b.w[0] = b.w[1] = b.w[2] = b.w[3] = 0; return b; }
static inline int big_bit(const Big &a, int i) { return (int)((a.w[i >> 6] >> (i & 63)) & 1); }
static inline void big_xor(Big &a, const Big &b) { for (int t = 0; t < 4; ++t) a.w[t] ^= b.w[t]; }
static inline Big big_shr2(const Big &a) {
    Big r;
    for (int t = 0; t < 4; ++t) r.w[t] = (a.w[t] >> 2) | (t < 3 ? a.w[t + 1] << 62 : 0);
    return r;
}
static inline Big big_mulz(const Big &a, const Big &plow, int n) {  // a * z in GF(2^n)
    const int top = big_bit(a, n - 1);
    Big r;
    for (int t = 3; t >= 0; --t) r.w[t] = (a.w[t] << 1) | (t > 0 ? a.w[t - 1] >> 63 : 0);
    for (int i = n; i < 256; ++i) r.w[i >> 6] &= ~(1ULL << (i & 63));
    if (top) big_xor(r, plow);
    return r;
}
static inline Big big_mul(Big a, const Big &b, const Big &plow, int n) {
    Big r = big_zero();
    for (int i = 0; i < n; ++i) {
        if (big_bit(b, i)) big_xor(r, a);
        a = big_mulz(a, plow, n);
    }
    return r;
}

// The bijective k-mer mapping (IBijectiveFunction / BijectiveKMapping in the reference: a random
// invertible GF(2) matrix): M = multiplication by a random element c of GF(2^2k), a universal
// family whose matrix is dense like a random one -- and because the k-mer window slides by one
// base (x' = (x >> 2) | b << (2k-2), i.e. x' = (x - low2) / z^2 + b z^(2k-2) as polynomials),
//     c*x' = (c*x + c*low2) * z^-2 + c*b*z^(2k-2),
// the scan kernels get the hash of the next window from the current one with one lookup in the
// 64-entry table roll[(h & 3) | out << 2 | in << 4] built here (key_limbs words per entry).
static int make_mapping(tsx_hip_map *m) {
    const int n = m->p.n, wk = m->p.wk;
    m->rows.assign((size_t)n * wk, 0);
    m->irows.assign((size_t)n * wk, 0);
    uint64_t st = m->seed;
    if (wk == 1) {
        const uint64_t plow = GF_POLY_LOW[n / 2], mask = (n < 64) ? ((1ULL << n) - 1ULL) : ~0ULL;
        uint64_t c = 0;
        while (c == 0 || c == 1) c = splitmix_next(st) & mask;       // 0 is not invertible, 1 is the identity
        // column j of M is c * z^j; rows[i] yields output bit n-1-i
        uint64_t col = c;
        for (int j = 0; j < n; ++j) {
            for (int r = 0; r < n; ++r)
                if ((col >> r) & 1ULL) rset(&m->rows[(size_t)(n - 1 - r)], j);
            col = gf_mulz(col, plow, n);
        }
        const uint64_t zinv = (plow >> 1) | (1ULL << (n - 1));       // z * zinv = 1 (P has constant term 1)
        const uint64_t zinv2 = gf_mul(zinv, zinv, plow, n);
        uint64_t A[4], C[4], E[4];
        for (int v = 0; v < 4; ++v) {
            A[v] = gf_mul(c, (uint64_t)v, plow, n);
            C[v] = A[v];
            for (int t = 0; t < n - 2; ++t) C[v] = gf_mulz(C[v], plow, n);
            E[v] = ((v & 1) ? zinv2 : 0ULL) ^ ((v & 2) ? zinv : 0ULL);
        }
        for (int idx = 0; idx < 64; ++idx) {
            const int hb = idx & 3, out = (idx >> 2) & 3, in = (idx >> 4) & 3;
            m->roll[idx] = (A[out] >> 2) ^ E[(hb ^ (int)(A[out] & 3ULL)) & 3] ^ C[in];
        }
        // mirror roll: h(rc x') = z^2 h(rc x) + c comp(in) - c comp(out) z^n, indexed by the top two bits of h(rc x)
        // (which z^2 pushes out: T[e] = e z^n reduced), out and in
        uint64_t T[4], D[4];
        for (int v = 0; v < 4; ++v) {
            T[v] = ((v & 1) ? plow : 0ULL) ^ ((v & 2) ? gf_mulz(plow, plow, n) : 0ULL);
            D[v] = gf_mulz(gf_mulz(C[v], plow, n), plow, n);
        }
        for (int idx = 0; idx < 64; ++idx) {
            const int hb = idx & 3, out = (idx >> 2) & 3, in = (idx >> 4) & 3;
            m->mroll[idx] = T[hb] ^ D[3 - out] ^ A[3 - in];
        }
    } else {
        const uint8_t *e = GF_POLY_EXP[n / 2 - 1];
        Big plow = big_zero();
        plow.w[0] = 1;
        for (int t = 0; t < 3; ++t) if (e[t]) plow.w[e[t] >> 6] |= 1ULL << (e[t] & 63);
        Big c = big_zero();
        bool trivial = true;
        while (trivial) {   // 0 is not invertible, 1 is the identity
            for (int t = 0; t < 4; ++t) c.w[t] = splitmix_next(st);
            for (int i = n; i < 256; ++i) c.w[i >> 6] &= ~(1ULL << (i & 63));
            trivial = (c.w[0] <= 1 && !c.w[1] && !c.w[2] && !c.w[3]);
        }
        // column j of M is c * z^j; rows[i] yields output bit n-1-i
        Big col = c;
        for (int j = 0; j < n; ++j) {
            for (int r = 0; r < n; ++r)
                if (big_bit(col, r)) rset(&m->rows[(size_t)(n - 1 - r) * wk], j);
            col = big_mulz(col, plow, n);
        }
        Big zinv = big_zero();                                         // z * zinv = 1 (P has constant term 1)
        for (int t = 0; t < 4; ++t) zinv.w[t] = (plow.w[t] >> 1) | (t < 3 ? plow.w[t + 1] << 63 : 0);
        zinv.w[(n - 1) >> 6] |= 1ULL << ((n - 1) & 63);
        const Big zinv2 = big_mul(zinv, zinv, plow, n);
        Big A[4], C[4], E[4];
        for (int v = 0; v < 4; ++v) {
            Big bv = big_zero(); bv.w[0] = (uint64_t)v;
            A[v] = big_mul(c, bv, plow, n);
            C[v] = A[v];
            for (int t = 0; t < n - 2; ++t) C[v] = big_mulz(C[v], plow, n);
            E[v] = big_zero();
            if (v & 1) big_xor(E[v], zinv2);
            if (v & 2) big_xor(E[v], zinv);
        }
        m->roll_wide.assign((size_t)64 * wk, 0);
        for (int idx = 0; idx < 64; ++idx) {
            const int hb = idx & 3, out = (idx >> 2) & 3, in = (idx >> 4) & 3;
            Big r = big_shr2(A[out]);
            big_xor(r, E[(hb ^ (int)(A[out].w[0] & 3ULL)) & 3]);
            big_xor(r, C[in]);
            for (int t = 0; t < wk; ++t) m->roll_wide[(size_t)idx * wk + t] = r.w[t];
        }
        // mirror roll, as for one-limb keys
        Big T[4], D[4];
        const Big plowz = big_mulz(plow, plow, n);
        for (int v = 0; v < 4; ++v) {
            T[v] = big_zero();
            if (v & 1) big_xor(T[v], plow);
            if (v & 2) big_xor(T[v], plowz);
            D[v] = big_mulz(big_mulz(C[v], plow, n), plow, n);
        }
        m->mroll_wide.assign((size_t)64 * wk, 0);
        for (int idx = 0; idx < 64; ++idx) {
            const int hb = idx & 3, out = (idx >> 2) & 3, in = (idx >> 4) & 3;
            Big r = T[hb];
            big_xor(r, D[3 - out]);
            big_xor(r, A[3 - in]);
            for (int t = 0; t < wk; ++t) m->mroll_wide[(size_t)idx * wk + t] = r.w[t];
        }
    }
    // Inverse by Gauss-Jordan on [A | I], A[r][c] = coefficient of input bit c in output bit r
    // (output bit r is produced by rows[n-1-r]).
    std::vector<uint64_t> A((size_t)n * wk), I((size_t)n * wk, 0);
    for (int r = 0; r < n; ++r) {
        memcpy(&A[(size_t)r * wk], &m->rows[(size_t)(n - 1 - r) * wk], (size_t)wk * 8);
        rset(&I[(size_t)r * wk], r);
    }
    for (int c = 0; c < n; ++c) {
        int piv = -1;
        for (int r = c; r < n; ++r) if (rbit(&A[(size_t)r * wk], c)) { piv = r; break; }
        if (piv < 0) return TSX_HIP_EINVAL;  // singular: cannot happen for c != 0 with P irreducible
        if (piv != c) for (int t = 0; t < wk; ++t) { std::swap(A[(size_t)piv * wk + t], A[(size_t)c * wk + t]); std::swap(I[(size_t)piv * wk + t], I[(size_t)c * wk + t]); }
        for (int r = 0; r < n; ++r)
            if (r != c && rbit(&A[(size_t)r * wk], c))
                for (int t = 0; t < wk; ++t) { A[(size_t)r * wk + t] ^= A[(size_t)c * wk + t]; I[(size_t)r * wk + t] ^= I[(size_t)c * wk + t]; }
    }
    // input bit c = XOR of the output bits in I[c]; irows[i] yields original bit n-1-i
    for (int c = 0; c < n; ++c) memcpy(&m->irows[(size_t)(n - 1 - c) * wk], &I[(size_t)c * wk], (size_t)wk * 8);
    return TSX_HIP_OK;
}

static void apply_rows(const tsx_hip_map *m, const std::vector<uint64_t> &rows, const uint64_t *x, uint64_t *out) {
    const int n = m->p.n, wk = m->p.wk;
    memset(out, 0, (size_t)wk * 8);
    for (int i = 0; i < n; ++i) {
        uint64_t acc = 0;
        for (int t = 0; t < wk; ++t) acc ^= rows[(size_t)i * wk + t] & x[t];
        if (__builtin_parityll(acc)) rset(out, n - 1 - i);
    }
}

// LUT[group][v] = A * (v << (g*group)): the mapping is linear, so A*x is the
// XOR of one table entry per g-bit group of x.
static void make_lut(const tsx_hip_map *m, const std::vector<uint64_t> &rows, std::vector<uint64_t> &lut) {
    const int wk = m->p.wk, g = m->p.g, groups = m->p.groups;
    lut.assign((size_t)groups * (1u << g) * wk, 0);
    std::vector<uint64_t> x(wk), y(wk);
    for (int grp = 0; grp < groups; ++grp)
        for (unsigned v = 0; v < (1u << g); ++v) {
            std::fill(x.begin(), x.end(), 0);
            const int bit = grp * g;
            x[bit >> 6] = (uint64_t)v << (bit & 63);
            x[wk - 1] &= m->p.top_mask;
            apply_rows(m, rows, x.data(), y.data());
            memcpy(&lut[((size_t)grp * (1u << g) + v) * wk], y.data(), (size_t)wk * 8);
        }
}

// One-limb keys: the mapping as a LUT by 4-bit groups, entry [grp * 16 + v] = M * ((v << 4 grp) & top_mask).  M is
// linear, so entry 0 of every group is 0 -- walk_part_kernel looks up all 16 groups of a masked window and relies on it.
static void make_lut4(const tsx_hip_map *m, std::vector<uint64_t> &lut4) {
    lut4.assign(256, 0);
    for (int grp = 0; grp < 16; ++grp)
        for (uint64_t v = 0; v < 16; ++v) {
            uint64_t x = (v << (4 * grp)) & m->p.top_mask, y = 0;
            apply_rows(m, m->rows, &x, &y);
            lut4[grp * 16 + v] = y;
        }
}

// ---- layout -------------------------------------------------------------------
static int derive_layout(tsx_hip_map *m, int k, int l, int s, int overflow_l, int shard_bits, int shard_index) {
    if (k < 1 || k > 127 || l < 4 || l > 36 || s < 0 || s > 32) return TSX_HIP_EINVAL;
    if (shard_bits < 0 || shard_bits > 3 || shard_index < 0 || shard_index >= (1 << shard_bits)) return TSX_HIP_EINVAL;
    if (2 * k <= l + shard_bits) return TSX_HIP_EINVAL;  // TSXHashMap.h:91-94, on the whole (sharded) table
    TableParams &p = m->p;
    p.k = k; p.l = l; p.n = 2 * k; p.wk = (2 * k + 63) / 64;
    p.lg = l + shard_bits; p.shard = (uint32_t)shard_index;
    p.R = std::min(l, 8);
    p.F = 2 * k - p.lg;
    const int KB = p.R + p.F;
    int W, C;
    if (s == 0) {
        W = (KB + 5 + 63) / 64;
        C = std::min(32, 64 * W - KB - (W > 1 ? 1 : 0));
    } else {
        C = s;
        W = (KB + C + 63) / 64;
        if (W > 1) W = (KB + C + 1 + 63) / 64;
    }
    const int lock = (W > 1) ? 1 : 0;
    p.K0 = 64 - C - lock;
    if (W > 4 || p.K0 < p.R || p.K0 > 63) return TSX_HIP_EINVAL;
    // all spilled func bits must fit limbs 1..W-1
    if (KB - p.K0 > 64 * (W - 1)) return TSX_HIP_EINVAL;
    p.W = W; p.C = C; p.cshift = 64 - C;
    p.k0mask = (p.K0 >= 64) ? ~0ULL : ((1ULL << p.K0) - 1ULL);
    p.lock_bit = lock ? (1ULL << p.K0) : 0ULL;
    p.slot_mask = (1ULL << l) - 1ULL;
    // a segment fits a CU's LDS: 128 KiB = 2^14 one-limb slots or 2^12 four-limb slots (96 KiB of three-limb slots).  Two-limb
    // slots: 2^12 = 64 KiB, so that TWO build workgroups of 512 threads share a CU and one sweeps while the other inserts
    // (k = 63: build 13.3 -> 11.8 ms; 2^13-slot segments when that would need more than 2^18 of them).  One-limb slots at
    // 64 KiB: build 4.41 -> 3.91 ms, but a radix level of 512 lists costs 0.5 ms more: 11.97 against 12.05 ms per step, not taken.
    const int smax = (W == 1) ? 14 : (W == 2) ? 13 : 12;
    p.S = std::min(l, (W == 2 && l - 12 <= 18) ? 12 : smax);
    if (const char *e = getenv("TSX_HIP_SEG_BITS")) p.S = std::min(l, std::min(smax, std::max(8, atoi(e))));
    p.seg_mask = (1ULL << p.S) - 1ULL;
    const uint64_t maxr = (1ULL << p.R) - 1ULL;
    p.max_reprobes = (uint32_t)std::min<uint64_t>(maxr, p.slot_mask);
    p.top_mask = (p.n & 63) ? ((1ULL << (p.n & 63)) - 1ULL) : ~0ULL;
    p.line_mask = 3;                 // FASTQ records (tsx_hip_set_record_lines)
    // LUT granularity: bytes when the table stays <= 32 KiB of LDS, nibbles otherwise
    const size_t lut8 = (size_t)((p.n + 7) / 8) * 256 * p.wk * 8;
    p.g = (lut8 <= (32u << 10)) ? 8 : 4;
    p.groups = (p.n + p.g - 1) / p.g;
    // secondary array: one entry per slot whose counter overflowed.  With the automatic (wide) counters that
    // is a handful of hot k-mers: 2^(l-8) entries; with explicit narrow --s counters many keys carry: 2^(l-4).
    // (It is cleared with the table whenever something carried: 1 GiB at l = 30 cost 0.23 ms per clear.)
    int ol = overflow_l ? overflow_l : std::max(10, (s == 0 && C >= 16) ? l - 8 : l - 4);
    if (ol < 4 || ol > 34) return TSX_HIP_EINVAL;
    p.sec_mask = (1ULL << ol) - 1ULL;
    tsx_hip_layout &L = m->lay;
    L.shard_bits = shard_bits; L.shard_index = shard_index;
    L.k = k; L.l = l; L.key_limbs = p.wk; L.entry_limbs = W; L.func_bits = p.F; L.reprobe_bits = p.R;
    L.count_bits = C; L.overflow_l = ol; L.max_reprobes = p.max_reprobes; L.slots = 1ULL << l;
    L.table_bytes = L.slots * (uint64_t)W * 8ULL;
    return TSX_HIP_OK;
}

extern "C" int tsx_hip_create(tsx_hip_map **out, int k, int l, int storagebits, int overflow_l,
                              uint64_t hash_seed, int device) {
    return tsx_hip_create_shard(out, k, l, storagebits, overflow_l, hash_seed, device, 0, 0);
}

extern "C" int tsx_hip_create_shard(tsx_hip_map **out, int k, int l, int storagebits, int overflow_l,
                                    uint64_t hash_seed, int device, int shard_bits, int shard_index) {
    if (!out) return TSX_HIP_EINVAL;
    *out = nullptr;
    std::unique_ptr<tsx_hip_map> owner(new tsx_hip_map());   // released into *out on success
    tsx_hip_map *m = owner.get();
    int rc = derive_layout(m, k, l, storagebits, overflow_l, shard_bits, shard_index);
    if (rc != TSX_HIP_OK) return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) {
        g_last_error = "no HIP device (the HIP path has no CPU fallback)";
        return TSX_HIP_ENODEVICE;
    }
    m->device = device; m->seed = hash_seed;
    if (const char *e = getenv("TSX_HIP_PATH")) m->path = atoi(e);
    if (const char *e = getenv("TSX_HIP_PIECE_BYTES")) {
        const long long v = atoll(e);
        if (v >= 256) { m->piece = ((size_t)v + 15) & ~(size_t)15; m->piece_fixed = true; }
    }
    // Host pieces large enough for the partitioned path to pay off (text >= table / 32),
    // between 64 MiB and 1 GiB of pinned staging per buffer.
    if (!m->piece_fixed) {
        const size_t want = (size_t)(m->lay.table_bytes / 16);
        m->piece = std::min<size_t>((size_t)1 << 30, std::max<size_t>(STAGE_PIECE_DEFAULT, want)) & ~(size_t)4095;
    }
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    m->cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    TSX_TRY(m->stream.create());
    TSX_TRY(m->clear_ev.create());
    TSX_TRY(m->join_ev.create());
    TableParams &p = m->p;
    TSX_TRY(m->table.alloc(m->lay.table_bytes));
    TSX_TRY(m->sec_keys.alloc((p.sec_mask + 1) * 8));
    TSX_TRY(m->sec_cnt.alloc((p.sec_mask + 1) * 8));
    TSX_TRY(m->stats.alloc(ST_N * sizeof(unsigned long long)));
    TSX_TRY(m->seg_dirty.alloc((size_t)(m->lay.slots >> p.S)));
    p.table = m->table.get(); p.sec_keys = m->sec_keys.get(); p.sec_cnt = m->sec_cnt.get();
    p.stats = m->stats.get(); p.seg_dirty = m->seg_dirty.get();
    TSX_TRY(m->d_carry.alloc(64));
    TSX_TRY(m->d_seg.alloc(64 * sizeof(unsigned long long)));
    rc = make_mapping(m);
    if (rc != TSX_HIP_OK) return rc;
    make_lut(m, m->rows, m->lut);
    make_lut(m, m->irows, m->ilut);
    TSX_TRY(m->d_lut.alloc(m->lut.size() * 8));
    TSX_TRY(m->d_ilut.alloc(m->ilut.size() * 8));
    HIP_TRY(hipMemcpy(m->d_lut.get(), m->lut.data(), m->lut.size() * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(m->d_ilut.get(), m->ilut.data(), m->ilut.size() * 8, hipMemcpyHostToDevice));
    p.lut = m->d_lut.get(); p.ilut = m->d_ilut.get(); p.roll = nullptr;
    {
        const void *src = (p.wk == 1) ? (const void *)m->roll : (const void *)m->roll_wide.data();
        const size_t bytes = (size_t)64 * p.wk * 8;
        // one-limb keys: the same mapping as a LUT by 4-bit groups (16 x 16 entries = 2 KiB) behind the roll
        // table -- walk_part_kernel has no LDS to spare for the 8-bit-group LUT (16 KiB)
        std::vector<uint64_t> lut4;
        if (p.wk == 1) make_lut4(m, lut4);
        // the mirror roll of the canonical walks behind both (MROLL1_AT / 64 * key_limbs words in, tsx_device.h)
        const void *msrc = (p.wk == 1) ? (const void *)m->mroll : (const void *)m->mroll_wide.data();
        TSX_TRY(m->d_roll.alloc(2 * bytes + lut4.size() * 8));
        HIP_TRY(hipMemcpy(m->d_roll.get(), src, bytes, hipMemcpyHostToDevice));
        if (!lut4.empty())
            HIP_TRY(hipMemcpy(m->d_roll.get() + 64, lut4.data(), lut4.size() * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(m->d_roll.get() + 64 * p.wk + lut4.size(), msrc, bytes, hipMemcpyHostToDevice));
        p.roll = m->d_roll.get();
    }
    rc = clear_impl(m, true);
    if (rc != TSX_HIP_OK) return rc;
    *out = owner.release();
    return TSX_HIP_OK;
}

extern "C" void tsx_hip_destroy(tsx_hip_map *m) { delete m; }

extern "C" int tsx_hip_get_layout(const tsx_hip_map *m, tsx_hip_layout *out) {
    if (!m || !out) return TSX_HIP_EINVAL;
    *out = m->lay;
    return TSX_HIP_OK;
}

// Zero the secondary array only when something ever carried into it (it is 1/16 of the table's slots).
__global__ __launch_bounds__(NT) void sec_clear_kernel(TableParams p, int force) {
    if (!force && p.stats[ST_CARRY] == 0) return;
    const uint64_t n2 = (p.sec_mask + 1) / 2;   // uint4 = two slots
    for (uint64_t i = (uint64_t)blockIdx.x * NT + threadIdx.x; i < n2; i += (uint64_t)gridDim.x * NT) {
        reinterpret_cast<uint4 *>(p.sec_keys)[i] = make_uint4(0, 0, 0, 0);
        reinterpret_cast<uint4 *>(p.sec_cnt)[i] = make_uint4(0, 0, 0, 0);
    }
}

// full: zero everything now (creation).  Otherwise the table itself is only MARKED clear when the next
// partitioned build can take care of it (m->fresh): that build writes every segment exactly once -- built,
// or zeroed when it has no keys -- and every other entry point zeroes the table first (ensure_zeroed).
static int clear_impl(tsx_hip_map *m, bool full) {
    HIP_TRY(hipSetDevice(m->device));
    join_foreign(m, false);
    if (full || !can_partition(m)) {
        HIP_TRY(hipMemsetAsync(m->p.table, 0, m->lay.table_bytes, m->stream.get()));
        m->fresh = false;
    } else {
        m->fresh = true;
    }
    hipLaunchKernelGGL(sec_clear_kernel, dim3(m->cus * 4), dim3(NT), 0, m->stream.get(), m->p, full ? 1 : 0);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemsetAsync(m->p.stats, 0, ST_N * sizeof(unsigned long long), m->stream.get()));
    HIP_TRY(hipMemsetAsync(m->p.seg_dirty, 0, (size_t)(m->lay.slots >> m->p.S), m->stream.get()));
    HIP_TRY(hipEventRecord(m->clear_ev.get(), m->stream.get()));
    m->clear_ev_set = true;
    m->used = false;   // (the counting mode stays)
    return TSX_HIP_OK;
}

// The table was cleared lazily and the caller is not a partitioned build: zero it now.
static int ensure_zeroed(tsx_hip_map *m, hipStream_t st) {
    if (!m->fresh) return TSX_HIP_OK;
    HIP_TRY(hipMemsetAsync(m->p.table, 0, m->lay.table_bytes, st));
    m->fresh = false;
    return TSX_HIP_OK;
}

extern "C" int tsx_hip_clear(tsx_hip_map *m) {
    if (!m) return TSX_HIP_EINVAL;
    return clear_impl(m, false);
}

// Canonical counting is chosen per table before anything is inserted: a table that mixed both modes would
// hold a k-mer under two keys.  A table sharded by slot range is filled by the exchanges, which have no canonical form.
extern "C" int tsx_hip_set_canonical(tsx_hip_map *m, int on) {
    if (!m || m->used || (on && m->p.lg != m->p.l)) return TSX_HIP_EINVAL;
    m->canon = on != 0;
    return TSX_HIP_OK;
}

extern "C" int tsx_hip_canonical(const tsx_hip_map *m) {
    if (!m) return TSX_HIP_EINVAL;
    return m->canon ? 1 : 0;
}

// The base rule does not change keys: it may change between calls, each call counts under the rule it finds.  A
// table sharded by slot range is filled by the exchanges, which have no base rule.
extern "C" int tsx_hip_set_base_rule(tsx_hip_map *m, int acgt_only, int min_qual_char) {
    if (!m || acgt_only < 0 || acgt_only > 1 || min_qual_char < 0 || min_qual_char > 255) return TSX_HIP_EINVAL;
    if ((acgt_only || min_qual_char) && m->p.lg != m->p.l) return TSX_HIP_EINVAL;
    m->p.acgt_only = (uint32_t)acgt_only;
    m->minq = (uint32_t)min_qual_char;
    return TSX_HIP_OK;
}

extern "C" int tsx_hip_get_base_rule(const tsx_hip_map *m, int *acgt_only, int *min_qual_char) {
    if (!m) return TSX_HIP_EINVAL;
    if (acgt_only) *acgt_only = m->p.acgt_only ? 1 : 0;
    if (min_qual_char) *min_qual_char = (int)m->minq;
    return TSX_HIP_OK;
}

// canonical tables and tables with a base rule: single-table and merge paths only (the exchanges refuse them)
static inline bool exch_refused(const tsx_hip_map *m) {
    if (m && (m->p.acgt_only || m->minq)) { g_last_error = "a table with a base rule: single-table and merge paths only"; return true; }
    return m && m->canon;
}

extern "C" int tsx_hip_canonical_host(int k, const uint64_t *kmers, size_t n, uint64_t *out) {
    if (k < 1 || k > 127 || ((!kmers || !out) && n)) return TSX_HIP_EINVAL;
    const int wk = (2 * k + 63) / 64;
    const uint64_t top = ((2 * k) & 63) ? ((1ULL << ((2 * k) & 63)) - 1ULL) : ~0ULL;
    for (size_t i = 0; i < n; ++i) {
        uint64_t x[4] = {0, 0, 0, 0};
        for (int t = 0; t < wk; ++t) x[t] = kmers[i * wk + t];
        x[wk - 1] &= top;
        switch (wk) {
            case 1: lex_canonical<1>(*reinterpret_cast<uint64_t(*)[1]>(x), 2 * k); break;
            case 2: lex_canonical<2>(*reinterpret_cast<uint64_t(*)[2]>(x), 2 * k); break;
            case 3: lex_canonical<3>(*reinterpret_cast<uint64_t(*)[3]>(x), 2 * k); break;
            default: lex_canonical<4>(x, 2 * k); break;
        }
        for (int t = 0; t < wk; ++t) out[i * wk + t] = x[t];
    }
    return TSX_HIP_OK;
}

static int read_stats(tsx_hip_map *m, unsigned long long *st) {
    HIP_TRY(hipMemcpyAsync(st, m->p.stats, ST_N * sizeof(unsigned long long), hipMemcpyDeviceToHost, m->stream.get()));
    HIP_TRY(hipStreamSynchronize(m->stream.get()));
    return TSX_HIP_OK;
}

extern "C" int tsx_hip_sync(tsx_hip_map *m) {
    if (!m) return TSX_HIP_EINVAL;
    HIP_TRY(hipSetDevice(m->device));
    join_foreign(m, true);
    unsigned long long st[ST_N];
    int rc = read_stats(m, st);
    if (rc != TSX_HIP_OK) return rc;
    if (st[ST_FAIL]) return TSX_HIP_EFULL;
    if (st[ST_SECFAIL]) return TSX_HIP_EOVERFLOW;
    if (st[ST_LOCKTO]) return TSX_HIP_ELOCK;   // an expired spin re-probes: the key may sit in two slots
    return TSX_HIP_OK;
}

static inline hipStream_t pick_stream(tsx_hip_map *m, void *stream) {
    hipStream_t st = stream ? (hipStream_t)stream : m->stream.get();
    if (st != m->stream.get()) {
        if (m->clear_ev_set) (void)hipStreamWaitEvent(st, m->clear_ev.get(), 0);   // behind the last tsx_hip_clear
        m->foreign = st;
    }
    return st;
}
// The map's own stream is about to touch what a caller's stream may still be working on: order it behind.
static inline void join_foreign(tsx_hip_map *m, bool host_wait) {
    if (!m->foreign) return;
    if (host_wait) {
        (void)hipStreamSynchronize(m->foreign);
        m->foreign = nullptr;
    } else if (m->join_ev.get() && hipEventRecord(m->join_ev.get(), m->foreign) == hipSuccess) {
        (void)hipStreamWaitEvent(m->stream.get(), m->join_ev.get(), 0);
    }
}
static inline int grid_for(const tsx_hip_map *m, uint64_t work_items, int per_cu) {
    uint64_t blocks = (work_items + NT - 1) / NT;
    uint64_t cap = (uint64_t)m->cus * per_cu;
    return (int)std::max<uint64_t>(1, std::min(blocks, cap));
}

#define DISPATCH_WK(m, CALL)                         \
    switch ((m)->p.wk) {                             \
        case 1: { constexpr int WKV = 1; CALL; } break; \
        case 2: { constexpr int WKV = 2; CALL; } break; \
        case 3: { constexpr int WKV = 3; CALL; } break; \
        default: { constexpr int WKV = 4; CALL; } break; \
    }
// The kernels that make hashed keys in two forms: CANV = canonical counting (tsx_hip_set_canonical) or not.
#define DISPATCH_CANON(m, CALL)                                                    \
    if ((m)->canon) { constexpr bool CANV = true; CALL; } else { constexpr bool CANV = false; CALL; }
// The scan front ends in two forms: BRV = a base rule is in effect for this launch (tsx_hip_set_base_rule) or not.
#define DISPATCH_BR(m, CALL)                                                                                           \
    if ((m)->p.acgt_only || (m)->qmap_cur) { constexpr bool BRV = true; CALL; } else { constexpr bool BRV = false; CALL; }

// ---- partitioned path: plan, scratch, launches ------------------------------------
static inline int rec_words(int wk) { return wk == 3 ? 4 : wk; }

// Two radix levels of at most 512 lists reach 2^18 segments (2^32 one-limb slots).  A larger table of one-limb keys and
// slots is built SLAB BY SLAB: a slab is the 2^18 segments that share the top slab_bits() bits of the home slot -- exactly
// what a shard of a multi-GPU table is to its GPU -- and count_slabs() walks the strip descriptions once per slab, keeping
// the slab's keys (the owner-filtered walk of the sharded path), then runs level 2 and the build for that slab.
static int max_seg_bits() {   // TSX_HIP_SLAB_SEGBITS: tests build small tables slab by slab
    static int v = 0;
    if (!v) { v = 18; if (const char *e = getenv("TSX_HIP_SLAB_SEGBITS")) v = std::min(18, std::max(9, atoi(e))); }
    return v;
}
static int slab_bits(const tsx_hip_map *m) {
    const TableParams &p = m->p;
    const int nsegbits = p.l - p.S;
    if (nsegbits <= max_seg_bits() || p.wk != 1 || p.W != 1 || p.lg != p.l) return 0;
    return nsegbits - max_seg_bits();
}
// Whether a text of n bytes goes into the table slab by slab (count_slabs): the partitioned path where it pays off.
static inline bool slab_build_wanted(const tsx_hip_map *m, size_t n) {
    return slab_bits(m) && (m->path == 2 || (m->path == 0 && n * 32 >= m->lay.table_bytes));
}
static bool can_partition(const tsx_hip_map *m) {
    const TableParams &p = m->p;
    const int nsegbits = p.l - p.S;
    if (nsegbits >= 1 && nsegbits <= (p.lg == p.l && p.wk == 1 && p.W == 1 ? max_seg_bits() : 18)) return true;  // two levels of <= 512 lists
    const int sb = slab_bits(m);
    return sb >= 1 && sb <= 4;
}

// ---- the geometry of the partitioned path, each rule written down once ----------------------------------------------------
// Radix bits of level 1 / level 2 for 2^nsegbits segments (b2 == 0: one level).  The fan-out per level is capped at 512:
// the histogram of the scan kernel and the ring staging live in LDS.
struct RadixBits { int b1, b2; };
static inline RadixBits radix_bits(int nsegbits) {
    const int b1 = std::min(9, (nsegbits <= 8) ? nsegbits : (nsegbits + 1) / 2);
    return RadixBits{b1, nsegbits - b1};
}
// Workgroups of level 2 per level-1 bucket, each with a sub-list per segment: a power of two (the build gives every sub-list 16 / cpr2 waves).
static inline uint32_t cpr2_for(int cus, RadixBits rb) {
    if (rb.b2 <= 0) return 1;
    uint32_t c = std::min<uint32_t>(8, std::max<uint32_t>(1, (uint32_t)(cus * 8) / (1u << rb.b1)));
    while (c & (c - 1)) c &= c - 1;
    return c;
}
static uint32_t level2_cpr(const tsx_hip_map *m) { return cpr2_for(m->cus, radix_bits(m->p.l - m->p.S)); }
// Ring depth of partition_ring_kernel (log2 words): PART_FLUSH-1 words may stay behind a flush, plus one batch of arrivals.
static inline uint32_t ring_bits(uint32_t nb) {
    const uint32_t mean = std::max<uint32_t>(1, RING_NT * PART_WPT / nb);
    uint32_t bits = 4;
    while ((1u << bits) < PART_FLUSH + 2 * mean && bits < 6) ++bits;
    return bits;
}
// A level 1 over RECEIVED keys (sharded entry points): 32-word rings -- 16 words may stay behind a flush, 8 arrive per batch.
static const uint32_t RECV_RING_BITS = 5;
// Dynamic LDS of partition_ring_kernel: per list a ring of 2^bits words + 36 bytes of cursors, limits and descriptors.
static inline size_t ring_lds_bytes(uint32_t nb, uint32_t bits) { return (size_t)nb * (((size_t)8 << bits) + 36); }
// Dynamic LDS of walk_part_kernel: per level-1 list a ring, flush descriptor, tail|head, cursor, job.
static inline size_t walk_lds_bytes(uint32_t nb1) { return (size_t)nb1 * (((size_t)8 << SP_CAPBITS) + 8 + 8 + 4 + 4); }
// Above this much LDS one workgroup fits a CU: the ring and walk kernels run with 1024 threads then (16 waves either way).
static const size_t ONE_WG_LDS = (size_t)80 << 10;

// Grow-only scratch: room for `need` bytes, an eighth + 4 KiB more when it has to be allocated anew.
template <typename B>
static int grow(hipStream_t st, B &buf, size_t need) { return buf.reserve(&st, need, need + need / 8 + 4096); }

// The deferred list of the map (local runs): room for every record of the pass in the worst case (skewed
// input whose keys all spill); only what is appended is ever touched.
static int ensure_deferred(tsx_hip_map *m, uint64_t maxrec, hipStream_t st) {
    const int rw = rec_words(m->p.wk);
    if (!m->d_def_n.get()) TSX_TRY(m->d_def_n.alloc(64));
    // (passes of billions of records: room for 2^28 of them -- what lands here is hot keys with their totals and the
    // spill of skewed lists; beyond the capacity records count as insert failures, reported by tsx_hip_sync)
    if (maxrec > ((uint64_t)1 << 30)) maxrec = std::max<uint64_t>((uint64_t)1 << 28, maxrec / 16);
    if (maxrec <= m->def_cap()) return TSX_HIP_OK;
    const size_t cap = maxrec + maxrec / 8 + 4096;
    int rc = m->d_def_rec.reserve(&st, (size_t)maxrec * rw * 8, cap * rw * 8);   // (waits before it frees)
    if (rc == TSX_HIP_OK) rc = m->d_def_cnt.alloc(cap * 8);
    if (rc != TSX_HIP_OK) { m->d_def_rec.reset(); m->d_def_cnt.reset(); }   // both or none
    return rc;
}

// The dynamic-LDS limits of the partition, walk and build kernels, once per map, hence per device: the attribute belongs
// to the device's copy of the kernel.  Every instantiation the launchers below can pick stands in one of these lists.
template <typename... K>
static int set_max_lds(int bytes, K... kernels) {
    for (const void *f : {(const void *)kernels...})
        HIP_TRY(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    return TSX_HIP_OK;
}
template <int RW>
static int set_ring_lds(int bytes) {
    return set_max_lds(bytes, partition_ring_kernel<RW>, partition_ring_kernel<RW, 1024>, partition_ring_kernel<RW, RING_NT, true>,
                       partition_ring_kernel<RW, 1024, true>);
}
template <int NTV>
static int set_walk_lds(int bytes) {
    return set_max_lds(bytes, walk_part_kernel<NTV>, walk_part_kernel<NTV, true>, walk_part_kernel<NTV, false, true>,
                       walk_part_kernel<NTV, true, true>);
}
static int set_partition_attrs(tsx_hip_map *m) {
    if (m->attr_done) return TSX_HIP_OK;
    const int big = 150 << 10, seg = (128 << 10) + (32 << 10);
    TSX_TRY(set_ring_lds<1>(big)); TSX_TRY(set_ring_lds<2>(big)); TSX_TRY(set_ring_lds<4>(big));
    TSX_TRY(set_walk_lds<SP_NT>(big)); TSX_TRY(set_walk_lds<1024>(big));
    TSX_TRY(set_max_lds(seg, build_segments_stream_kernel<false>, build_segments_stream_kernel<true>,
                        build_segments_wide_stream_kernel<1>, build_segments_wide_stream_kernel<2>,
                        build_segments_wide_stream_kernel<3>, build_segments_wide_stream_kernel<4>));
    TSX_TRY(set_max_lds(64 << 10, walk_log_wide_kernel<3>, walk_log_wide_kernel<4>, walk_log_wide_kernel<3, true>,
                        walk_log_wide_kernel<4, true>));
    m->attr_done = true;
    return TSX_HIP_OK;
}

// maxrec: upper bound of records; g: number of source regions; own_log: the records come from
// this map's scan kernel (needs the log buffer); hist_nb_override: sharded scan.
static int plan_partition(tsx_hip_map *m, uint64_t maxrec, int g, bool own_log, uint32_t hist_nb_override,
                          hipStream_t st, PartPlan &pl, int fused_g = 0) {
    const TableParams &p = m->p;
    const int nsegbits = p.l - p.S;
    pl.g = g;
    pl.rw = rec_words(p.wk);
    pl.nseg = 1u << nsegbits;
    const RadixBits rb = radix_bits(nsegbits);
    pl.b1 = rb.b1; pl.b2 = rb.b2;
    pl.nb1 = 1u << pl.b1; pl.nb2 = 1u << pl.b2;
    pl.hist_nb = hist_nb_override ? hist_nb_override : pl.nb1;
    auto even = [](uint64_t v) { return (v + 1) & ~1ULL; };
    pl.log_cap = even(maxrec / g + maxrec / g / 3 + 2048);
    if (const char *e = getenv("TSX_HIP_LOG_CAP")) pl.log_cap = even(std::max(16, atoi(e)));  // tests: force region overflow
    pl.cpr2 = cpr2_for(m->cus, rb);
    if (pl.b2) if (const char *e = getenv("TSX_HIP_CPR2")) pl.cpr2 = (uint32_t)std::min(8, std::max(1, atoi(e)));
    const uint64_t per_sub = maxrec / pl.nseg / pl.cpr2;
    // multiple of 16 records: every sub-list starts on a 128-B line
    pl.cap_sub = (per_sub + per_sub / 4 + 6 * (uint64_t)std::sqrt((double)per_sub + 1.0) + 64 + 15) & ~15ULL;
    // fused scan + level 1: one-limb keys, two levels (a one-level split feeds the build, which takes <= 8 pieces)
    pl.fused = fused_g > 0 && pl.b2 > 0 && p.wk == 1 && (fused_g + pl.cpr2 - 1) / pl.cpr2 <= (uint32_t)PART_MAX_PIECES;
    pl.G1 = pl.fused ? (uint32_t)fused_g : 0;
    pl.cap1 = 0;
    pl.l1_wgm = false;   // (whoever fills the lists says otherwise: scan_fused)
    if (pl.fused) {
        const uint64_t per1 = maxrec / pl.nb1 / pl.G1;
        pl.cap1 = (per1 + per1 / 4 + 6 * (uint64_t)std::sqrt((double)per1 + 1.0) + 64 + 15) & ~15ULL;
        if (const char *e = getenv("TSX_HIP_CAP1")) pl.cap1 = (uint64_t)std::max(16, atoi(e) & ~15);   // tests: force overflow
    }
    // buffer 0: key log, later the segment sub-lists of a two-level split; buffer 1: packed level-1 output, or the
    // level-1 sub-lists of the fused scan
    const uint64_t rec_cap = pl.fused ? 0 : (own_log ? (uint64_t)g * pl.log_cap : maxrec);
    const size_t need0 = std::max<uint64_t>(own_log ? rec_cap : 0, pl.b2 ? (uint64_t)pl.nseg * pl.cpr2 * pl.cap_sub : 0) * 8 * pl.rw;
    const size_t need1 = (pl.fused ? (uint64_t)pl.nb1 * pl.G1 * pl.cap1 : rec_cap) * 8 * pl.rw;
    TSX_TRY(grow(st, m->d_buf[0], need0));
    TSX_TRY(grow(st, m->d_buf[1], need1));
    pl.buf1 = m->d_buf[1].get();
    // counters: [region fill | region start | bucket start | bucket size | sub-list size], then the
    // histogram matrix (u32) and its exclusive scan (u64), both max(nb1, hist_nb) x g
    const uint32_t hb = std::max(pl.nb1, pl.hist_nb);
    pl.cnt_need = 2 * (size_t)g + 2 * (size_t)hb + (size_t)pl.nseg * pl.cpr2 + (size_t)pl.nb1 * pl.G1;
    const size_t mat = (size_t)hb * g;
    TSX_TRY(grow(st, m->d_cnt, pl.cnt_need * 8 + mat * 12 + 64));
    pl.c_log = m->d_cnt.get();                    // fill of each log region, or size of each cut of a received array
    pl.c_rstart = pl.c_log + g;
    pl.c_bstart = pl.c_rstart + g; pl.c_bcnt = pl.c_bstart + hb; pl.c_seg = pl.c_bcnt + hb;
    pl.c_l1 = pl.c_seg + (size_t)pl.nseg * pl.cpr2;
    pl.d_offs = pl.c_l1 + (size_t)pl.nb1 * pl.G1;
    pl.d_hist = reinterpret_cast<uint32_t *>(pl.d_offs + mat);
    HIP_TRY(hipMemsetAsync(m->d_cnt.get(), 0, pl.cnt_need * 8, st));
    TSX_TRY(set_partition_attrs(m));
    return TSX_HIP_OK;
}

// One launch of walk_part_kernel.  The form is picked from the launch's own arguments: LOCAL for what a plain one-GPU
// count passes (walk_local_form, tsx_partition.h), the general form for everything else; 1024 threads where 512 lists
// leave room for one workgroup per CU.
// The launch records below carry the kernel's own parameter names, in the kernel's order; a field left alone is the
// "absent" value (null, 0, one piece).  Each kernel family has ONE launcher that hands the fields over.
struct WalkPartLaunch {
    uint32_t grid = 0;
    const uint4 *desc = nullptr; uint64_t desc_cap = 0; const unsigned long long *desc_cnt = nullptr; uint32_t nregions = 0;
    uint64_t *dst = nullptr; uint64_t dst_cap = 0; unsigned long long *dst_cnt = nullptr; uint32_t nb = 0, shift = 0;
    uint64_t *ovq_all = nullptr; uint32_t *ovq_cnt = nullptr; uint32_t ovq_cap = 0; uint64_t n_packed = 0;
    uint32_t dst_g0 = 0, dst_gtot = 0; int own_flags = 0; unsigned long long *emit_sum = nullptr; int long_desc = 0; uint32_t flush_q = 0;
    int dst_wgm = 0;   // set by launch_walk_part: the lists are numbered workgroup-major (tsx_layout.h) -- the LOCAL form, and it alone
};
static void launch_walk_part(tsx_hip_map *m, hipStream_t st, const TableParams &pp, WalkPartLaunch &a) {
    const size_t lds = walk_lds_bytes(a.nb);
#define TSX_WALK(NTV, CANV, LOCV)                                                                                              \
    hipLaunchKernelGGL((walk_part_kernel<NTV, CANV, LOCV>), dim3(a.grid), dim3(NTV), lds, st, pp, a.desc, a.desc_cap,          \
                       a.desc_cnt, a.nregions, a.dst, a.dst_cap, a.dst_cnt, a.nb, a.shift, a.ovq_all, a.ovq_cnt, a.ovq_cap,    \
                       a.n_packed, a.dst_g0, a.dst_gtot, a.own_flags, a.emit_sum, a.long_desc, a.flush_q, a.dst_wgm)
    const bool local = walk_local_form(a.own_flags, a.n_packed, a.long_desc, a.flush_q, a.emit_sum, a.dst_g0);
    // The LOCAL form fills all G lists of every bucket in one launch and nothing is appended to them later: it keeps a
    // workgroup's lists side by side.  The general form fills list sets launch by launch and stays bucket-major.
    a.dst_wgm = local ? 1 : 0;
    if (lds > ONE_WG_LDS) {   // 512 lists
        if (local) { DISPATCH_CANON(m, TSX_WALK(1024, CANV, true)); } else { DISPATCH_CANON(m, TSX_WALK(1024, CANV, false)); }
    } else {
        if (local) { DISPATCH_CANON(m, TSX_WALK(SP_NT, CANV, true)); } else { DISPATCH_CANON(m, TSX_WALK(SP_NT, CANV, false)); }
    }
#undef TSX_WALK
}

// Launch with the record width as a compile-time constant.
#define DISPATCH_RW(rw, CALL)                        \
    switch (rw) {                                    \
        case 1: { constexpr int RWV = 1; CALL; } break; \
        case 2: { constexpr int RWV = 2; CALL; } break; \
        default: { constexpr int RWV = 4; CALL; } break; \
    }

// One launch of partition_ring_kernel: the only dispatch over the record width, the workgroup size and SKEW.
struct RingLaunch {
    uint32_t grid = 0;
    int rw = 1;               // words per record
    bool skew = false;        // the SKEW form (level 2)
    bool fixed_nt = false;    // RING_NT threads whatever the rings take (a level 1 over received keys); else 1024 above ONE_WG_LDS
    const uint64_t *src = nullptr; const unsigned long long *src_start = nullptr, *src_cnt = nullptr; uint64_t src_cap = 0;
    uint32_t nregions = 0, cpr = 1; uint64_t *dst = nullptr; const unsigned long long *offs = nullptr, *offs_base = nullptr;
    unsigned long long *dst_cnt = nullptr; uint64_t dst_cap = 0; uint32_t nb = 0, shift = 0, capbits = 0;
    uint64_t *ovq_all = nullptr; uint32_t *ovq_cnt = nullptr; uint32_t ovq_cap = 0;
    const unsigned long long *src_pcnt = nullptr; uint32_t src_np = 0; uint64_t src_pcap = 0;
    int src_wgm = 0;          // the pieces are sub-lists numbered workgroup-major (tsx_layout.h): what follows a LOCAL walk
    int dst_bm = 0;
    unsigned long long *key_sum = nullptr; uint32_t dst_r0 = 0, dst_nr = 0; int fmt = 0; uint32_t dch = 0; const uint32_t *skew_flag = nullptr;
};
static void launch_ring(hipStream_t st, const TableParams &pp, const RingLaunch &a) {
    const size_t lds = ring_lds_bytes(a.nb, a.capbits);
#define TSX_RING(RWV, NTV, SK)                                                                                                 \
    hipLaunchKernelGGL((partition_ring_kernel<RWV, NTV, SK>), dim3(a.grid), dim3(NTV), lds, st, pp, a.src, a.src_start,        \
                       a.src_cnt, a.src_cap, a.nregions, a.cpr, a.dst, a.offs, a.offs_base, a.dst_cnt, a.dst_cap, a.nb,        \
                       a.shift, a.capbits, a.ovq_all, a.ovq_cnt, a.ovq_cap, a.src_pcnt, a.src_np, a.src_pcap, a.src_wgm,       \
                       a.dst_bm, a.key_sum, a.dst_r0, a.dst_nr, a.fmt, a.dch, a.skew_flag)
    // (512 lists: the rings leave room for one workgroup per CU -- 1024 threads then, 16 waves either way)
    if (!a.fixed_nt && lds > ONE_WG_LDS) {
        if (a.skew) { DISPATCH_RW(a.rw, TSX_RING(RWV, 1024, true)); } else { DISPATCH_RW(a.rw, TSX_RING(RWV, 1024, false)); }
    } else {
        if (a.skew) { DISPATCH_RW(a.rw, TSX_RING(RWV, RING_NT, true)); } else { DISPATCH_RW(a.rw, TSX_RING(RWV, RING_NT, false)); }
    }
#undef TSX_RING
}

// walk_log_kernel (one-limb keys) / walk_log_wide_kernel (the last four fields do not exist there and stay absent).
struct WalkLogLaunch {
    uint32_t grid = 0;
    const uint4 *desc = nullptr; uint64_t desc_cap = 0; const unsigned long long *desc_cnt = nullptr; uint32_t nregions = 0;
    uint64_t *log = nullptr; uint64_t log_cap = 0; unsigned long long *log_cnt = nullptr; uint32_t *hist = nullptr;
    uint32_t hist_nb = 0, hist_shift = 0; uint64_t n_packed = 0; int long_desc = 0, own_only = 0; unsigned long long *emit_sum = nullptr;
};
static void launch_walk_log(tsx_hip_map *m, hipStream_t st, const TableParams &pp, const WalkLogLaunch &a) {
    const size_t lut_bytes = m->lut.size() * 8;
#define TSX_WALK_WIDE(WKV)                                                                                                     \
    DISPATCH_CANON(m, hipLaunchKernelGGL((walk_log_wide_kernel<WKV, CANV>), dim3(a.grid), dim3(NT), lut_bytes, st, pp, a.desc, \
                                         a.desc_cap, a.desc_cnt, a.nregions, a.log, a.log_cap, a.log_cnt, a.hist, a.hist_nb,   \
                                         a.hist_shift))
    switch (m->p.wk) {
        case 1:
            DISPATCH_CANON(m, hipLaunchKernelGGL((walk_log_kernel<CANV>), dim3(a.grid), dim3(NT), lut_bytes, st, pp, a.desc,
                                                 a.desc_cap, a.desc_cnt, a.nregions, a.log, a.log_cap, a.log_cnt, a.hist,
                                                 a.hist_nb, a.hist_shift, a.n_packed, a.long_desc, a.own_only, a.emit_sum));
            break;
        case 2: TSX_WALK_WIDE(2); break;
        case 3: TSX_WALK_WIDE(3); break;
        default: TSX_WALK_WIDE(4); break;
    }
#undef TSX_WALK_WIDE
}

// The window-wise level 1 of a sharded run plans with its own sub-list buffer and counters in the map's place.
static int plan_sharded_l1(tsx_hip_map *m, uint64_t maxrec, int g1, hipStream_t st, PartPlan &pl) {
    std::swap(m->d_buf[1], m->sh_buf1); std::swap(m->d_cnt, m->sh_cnt);
    const int rc = plan_partition(m, maxrec, g1, false, 0, st, pl, g1);
    std::swap(m->d_buf[1], m->sh_buf1); std::swap(m->d_cnt, m->sh_cnt);
    return rc;
}

// Overflow queues (OVQ_CAP records each): one per level-2 workgroup, plus one per workgroup of the fused scan.
static int ensure_ovq(tsx_hip_map *m, size_t nq, int rw, hipStream_t st) {
    const size_t bytes = nq * OVQ_CAP * 8 * rw;
    if (bytes <= m->d_ovq.cap()) return TSX_HIP_OK;
    int rc = m->d_ovq.reserve(&st, bytes, bytes);   // (waits before it frees)
    if (rc == TSX_HIP_OK) rc = m->d_ovq_cnt.alloc(nq * 4 + 512 * 4 + 64);   // (+ the skew flags of level 2, one per bucket, behind the counters)
    if (rc != TSX_HIP_OK) { m->d_ovq.reset(); m->d_ovq_cnt.reset(); }   // both or none
    return rc;
}
// queues of a map whose records are rw words wide (the skew flags lie behind their counters)
static inline size_t ovq_queues(const tsx_hip_map *m, int rw) { return m->d_ovq.cap() / ((size_t)OVQ_CAP * 8 * rw); }

// Level-1 lists per slot of a sharded step: two workgroups per CU while the pieces of a bucket stay within what a
// level-2 workgroup walks.
static uint32_t shard_lists_per_slot(const tsx_hip_map *m, uint32_t nslots) {
    uint32_t gw = (uint32_t)m->cus * 2;
    while (gw > 32 && (uint64_t)gw * nslots > (uint64_t)PART_MAX_PIECES * level2_cpr(m)) gw /= 2;
    return gw;
}
// The sharded level 1 of a step, window by window (or slot by slot).  first: the step begins -- plan `sets` sets of `rw`
// lists for maxrec records into sh_pl, make room in the deferred list and the overflow queues, clear their counters, and
// remember the step's shape; a later window or slot must find that shape (`windows`) and a fused plan.
static int sharded_l1_step(tsx_hip_map *m, bool first, uint32_t rw, uint32_t sets, uint32_t windows, uint64_t maxrec,
                           hipStream_t st) {
    if (!m->sh_pl) m->sh_pl.reset(new PartPlan());
    PartPlan &pl = *m->sh_pl;
    if (!first) return (m->sh_windows != windows || !pl.fused) ? TSX_HIP_EINVAL : TSX_HIP_OK;
    m->sh_rw = rw;
    m->sh_windows = windows;
    TSX_TRY(plan_sharded_l1(m, maxrec, (int)(rw * sets), st, pl));
    if (!pl.fused) return TSX_HIP_EINVAL;
    TSX_TRY(ensure_deferred(m, maxrec, st));
    HIP_TRY(hipMemsetAsync(m->d_def_n.get(), 0, 8, st));
    const size_t nq = (size_t)pl.nb1 * pl.cpr2 + pl.G1;
    TSX_TRY(ensure_ovq(m, nq, pl.rw, st));
    HIP_TRY(hipMemsetAsync(m->d_ovq_cnt.get(), 0, nq * 4, st));   // (also the queues of windows that never run)
    return TSX_HIP_OK;
}
// A level 1 over received one-limb keys: `grid` workgroups, each with a fixed-capacity sub-list per bucket among the
// plan's G1 (as level 2 keeps them -- no histogram pass) and an overflow queue, the first of them queue `list0` behind
// level 2's.  The caller names the source and which lists the workgroups fill (dst_r0, dst_nr).
static RingLaunch recv_level1(const tsx_hip_map *m, const PartPlan &pl, uint32_t grid, uint32_t list0) {
    RingLaunch r;
    r.grid = grid; r.fixed_nt = true;
    r.dst = pl.buf1; r.dst_cnt = pl.c_l1; r.dst_cap = pl.cap1;
    r.nb = pl.nb1; r.shift = (uint32_t)(m->p.l - pl.b1); r.capbits = RECV_RING_BITS;
    const size_t q0 = (size_t)pl.nb1 * pl.cpr2 + list0;
    r.ovq_all = m->d_ovq.get() + q0 * OVQ_CAP; r.ovq_cnt = m->d_ovq_cnt.get() + q0; r.ovq_cap = OVQ_CAP;
    r.dst_bm = 1;
    return r;
}

// Radix level 1 (+ level 2), the segment build, then everything that waited for the build (overflow
// queues, deferred list).  Source records: g regions of `src`, either src_cap apart with fills c_log (a
// key log) or at region_start/c_log (cuts of a packed array); pl.d_hist must hold their level-1
// histogram.  The caller has made room in the map's deferred list (ensure_deferred) and reset its
// counter before the first kernel that may append to it.
static int run_partition_build(tsx_hip_map *m, const PartPlan &pl, const uint64_t *src,
                               const unsigned long long *region_start, uint64_t src_cap, hipStream_t st,
                               Event *ev = nullptr) {
    TableParams pp = m->p;
    const TableParams &p = m->p;
    pp.defer = m->defer();
    const int rw = pl.rw;
    if (!pl.fused) {
    hipLaunchKernelGGL(offsets_rows_kernel, dim3(pl.nb1), dim3(1024), 0, st, (const uint32_t *)pl.d_hist, pl.d_offs,
                       (uint32_t)pl.g, pl.c_bcnt);
    hipLaunchKernelGGL(offsets_finish_kernel, dim3(1), dim3(1024), 0, st, pl.nb1, pl.c_bstart, pl.c_bcnt);
    {   // level 1: every region -> packed array ordered by the top b1 bits of the home slot
        RingLaunch r;
        r.grid = (uint32_t)pl.g; r.rw = rw;
        r.src = src; r.src_start = region_start; r.src_cnt = pl.c_log; r.src_cap = src_cap; r.nregions = (uint32_t)pl.g;
        r.dst = pl.buf1; r.offs = pl.d_offs; r.offs_base = pl.c_bstart;
        r.nb = pl.nb1; r.shift = (uint32_t)(p.l - pl.b1); r.capbits = ring_bits(pl.nb1);
        launch_ring(st, pp, r);
        HIP_TRY(hipGetLastError());
    }
    }   // (fused: walk_part_kernel has left the level-1 sub-lists in buffer 1)
    if (ev) HIP_TRY(hipEventRecord(ev[EV_L1_END].get(), st));
    const uint64_t *lists = pl.buf1;
    const unsigned long long *lists_start = pl.c_bstart, *lists_cnt = pl.c_bcnt;
    uint64_t lists_cap = 0;
    uint32_t pieces = 1;
    uint32_t nq2 = 0;
    // level 2 leaves PRE-FORMATTED records (format_record, tsx_partition.h) where the stream build of one-limb keys and
    // slots reads them and the fields fit: slot image in bits [0, R + F), first probe position above
    const int pre = (pl.b2 && p.wk == 1 && p.W == 1 && p.R + p.F >= 32 && p.R + p.F + p.S <= 64) ? 1 : 0;
    if (pl.b2) {  // level 2: cpr2 workgroups per level-1 bucket, each with its own sub-list per segment
        nq2 = pl.nb1 * pl.cpr2;   // one overflow queue per workgroup (the fused scan's queues follow them)
        // records per private chunk of the deferred list (mass spills of skewed input, see partition_ring_kernel): a
        // quarter of the list shared out over the workgroups, a power of two in 64 .. 4096; 0: the list is too small
        uint32_t dch = 0;
        for (uint32_t c = 4096; c >= 64 && !dch; c >>= 1)
            if ((uint64_t)c * nq2 * 4 <= m->def_cap()) dch = c;
        {
            const int rco = ensure_ovq(m, (size_t)nq2 + pl.G1, rw, st);
            if (rco != TSX_HIP_OK) return rco;
        }
        // Which form of the level-2 kernel works (partition_ring_kernel: SKEW) is decided on the device: skew_probe_kernel
        // samples every bucket and raises the flag -- the last word of the overflow-queue counters -- when it finds a hot
        // key; both forms are launched, per bucket one of them returns at once.
        uint32_t *d_skew = m->d_ovq_cnt.get() + ovq_queues(m, rw);   // (ensure_ovq keeps one spare counter behind the queues')
        DISPATCH_RW(rw, hipLaunchKernelGGL((skew_probe_kernel<RWV>), dim3(pl.nb1), dim3(256), 0, st, (const uint64_t *)pl.buf1,
                                           (const unsigned long long *)pl.c_bstart, (const unsigned long long *)pl.c_bcnt,
                                           (const unsigned long long *)(pl.fused ? pl.c_l1 : nullptr), pl.G1, pl.cap1,
                                           pl.l1_wgm ? 1 : 0, d_skew));
        RingLaunch r;
        r.grid = pl.nb1 * pl.cpr2; r.rw = rw;
        r.src = pl.buf1; r.src_start = pl.c_bstart; r.src_cnt = pl.c_bcnt; r.nregions = pl.nb1; r.cpr = pl.cpr2;
        r.dst = m->d_buf[0].get(); r.dst_cnt = pl.c_seg; r.dst_cap = pl.cap_sub;
        r.nb = pl.nb2; r.shift = (uint32_t)p.S; r.capbits = ring_bits(pl.nb2);
        r.ovq_all = m->d_ovq.get(); r.ovq_cnt = m->d_ovq_cnt.get(); r.ovq_cap = OVQ_CAP;
        r.src_pcnt = pl.fused ? pl.c_l1 : nullptr; r.src_np = pl.G1; r.src_pcap = pl.cap1; r.src_wgm = pl.l1_wgm ? 1 : 0;
        r.fmt = pre; r.dch = dch; r.skew_flag = d_skew;
        launch_ring(st, pp, r);
        r.skew = true;
        launch_ring(st, pp, r);
        HIP_TRY(hipGetLastError());
        lists = m->d_buf[0].get(); lists_start = nullptr; lists_cnt = pl.c_seg; lists_cap = pl.cap_sub; pieces = pl.cpr2;
    }
    if (ev) HIP_TRY(hipEventRecord(ev[EV_L2_END].get(), st));
    const int fresh = m->fresh ? 1 : 0;
    const int gb = (int)std::min<uint32_t>(pl.nseg, (uint32_t)m->cus * 16);
    const size_t seg_bytes = ((size_t)8 << p.S) * p.W;
    if (p.wk == 1 && p.W == 1) {   // 1024 threads: the segment + 16 waves' rings of 2 KiB
        const size_t lds = seg_bytes + (size_t)(1024 / 64) * 2048;
        if (pre)
            hipLaunchKernelGGL((build_segments_stream_kernel<true>), dim3(gb), dim3(1024), lds, st, pp,
                               lists, lists_start, lists_cnt, lists_cap, pieces, pl.nseg, fresh);
        else
            hipLaunchKernelGGL((build_segments_stream_kernel<false>), dim3(gb), dim3(1024), lds, st, pp,
                               lists, lists_start, lists_cnt, lists_cap, pieces, pl.nseg, fresh);
    } else {   // multi-limb keys and / or slots: wave streams too (64 records of LDS per wave behind the segment)
        // a segment of <= 64 KiB (TSX_HIP_SEG_BITS): 512 threads, two workgroups per CU -- one sweeps while the other inserts
        const int wnt = (seg_bytes <= ((size_t)64 << 10)) ? 512 : 1024;
        const size_t ring_bytes = (size_t)(wnt / 64) * 64 * 8 * rw;
        DISPATCH_WK(m, hipLaunchKernelGGL((build_segments_wide_stream_kernel<WKV>), dim3(gb), dim3(wnt),
                                          seg_bytes + ring_bytes, st, pp, lists, lists_start, lists_cnt, lists_cap, pieces,
                                          pl.nseg, fresh));
    }
    HIP_TRY(hipGetLastError());
    m->fresh = false;   // every segment has been written: built, or zeroed
    if (ev) HIP_TRY(hipEventRecord(ev[EV_BUILD_END].get(), st));
    // Records that found their sub-list filled up by a hot key, and the deferred list: inserted now, by the
    // whole chip, into a table whose segments are all in place.
    if (nq2) {
        const uint32_t nq = nq2 + pl.G1;
        DISPATCH_WK(m, hipLaunchKernelGGL((overflow_insert_kernel<WKV>), dim3(std::min<uint32_t>(nq, (uint32_t)m->cus * 8)),
                                          dim3(PART_NT), 0, st, pp, (const uint64_t *)m->d_ovq.get(),
                                          (const uint32_t *)m->d_ovq_cnt.get(), OVQ_CAP, nq));
        HIP_TRY(hipGetLastError());
    }
    DISPATCH_WK(m, hipLaunchKernelGGL((deferred_insert_kernel<WKV>), dim3(m->cus * 2), dim3(PART_NT), 0, st, pp,
                                      (const uint64_t *)m->d_def_rec.get(), (const uint64_t *)m->d_def_cnt.get(),
                                      (const unsigned long long *)m->d_def_n.get(), (uint64_t)0, m->def_cap()));
    HIP_TRY(hipGetLastError());
    return TSX_HIP_OK;
}

struct HotOut { uint64_t *keys = nullptr, *cnts = nullptr; uint64_t cap = 0; unsigned long long *n = nullptr; };
// Sharded scan: where the keys go.  send: groups by owner GPU (own group left out when `own` is given),
// own: this GPU's keys (they never travel), counts[o]: keys per owner, key_sum += sum of all keys.
struct ShardOut {
    uint64_t *send = nullptr; uint64_t send_cap = 0;
    uint64_t *own = nullptr; uint64_t own_cap = 0;
    unsigned long long *counts = nullptr, *key_sum = nullptr;
};

// One FASTQ piece already on the device: passes 1-3.  own_end = number of start
// positions this piece owns (bytes past it are halo for windows that begin
// before it); head_open = the piece starts in the middle of a line.
// shard_send != nullptr: sharded scan -- the keys are not built into the local table but
// split by owner into shard_send (counts per owner to shard_counts), hot keys to `hot`.
// Sharded run, description exchange: the piece is only DESCRIBED (strip_desc_kernel), the descriptions packed
// into out[0 .. *count).
// owners > 0 (minimizer exchange): one packed list per owner GPU at out + o * cap, count[0 .. owners) their lengths,
// count[owners .. owners + 4) the homopolymer k-mer occurrences taken out of the descriptions, per base.
struct DescOut { uint4 *out = nullptr; uint64_t cap = 0; unsigned long long *count = nullptr, *sum = nullptr; int long_desc = 0; int owners = 0; };
// (owners != 0: describe only -- the wave regions stay in buffer 1 for mini_split)

// Room for the line counts of ntiles tiles and one partial sum per SCAN_CHUNK of them behind m->tile_cap counts.
static int ensure_tiles(tsx_hip_map *m, uint64_t ntiles, hipStream_t st) {
    if (ntiles <= m->tile_cap) return TSX_HIP_OK;
    const uint64_t cap = ntiles + ntiles / 4 + 1024;
    const size_t bytes = (size_t)(cap + cap / SCAN_CHUNK + 16) * sizeof(uint32_t);
    m->tile_cap = 0;
    TSX_TRY(m->d_tile.reserve(&st, bytes, bytes));
    m->tile_cap = cap;
    return TSX_HIP_OK;
}

// ---- stage timing: tuples of EV_N events (TimingEvent) on the launch stream ----------------------------------------------
// The next tuple of the map (its events are created on first use).
static int next_timing_events(tsx_hip_map *m, Event *&ev) {
    while (m->ev_used + EV_N > m->ev.size()) {
        m->ev.emplace_back();
        const int rc = m->ev.back().create(hipEventDefault);
        if (rc != TSX_HIP_OK) { m->ev.pop_back(); return rc; }
    }
    ev = &m->ev[m->ev_used]; m->ev_used += EV_N;
    return TSX_HIP_OK;
}
// Events first .. last of a tuple, back to back.
static int timing_record(Event *ev, int first, int last, hipStream_t st) {
    for (int i = first; i <= last; ++i) HIP_TRY(hipEventRecord(ev[i].get(), st));
    return TSX_HIP_OK;
}
// Opens a tuple and records its first event; ev stays null where timing is off, and every helper below takes that.
static int timing_open(tsx_hip_map *m, Event *&ev, hipStream_t st) {
    ev = nullptr;
    if (!m->timing) return TSX_HIP_OK;
    TSX_TRY(next_timing_events(m, ev));
    return timing_record(ev, EV_BEGIN, EV_BEGIN, st);
}
// Nothing more of the tuple happens in this call: every event from `from` to the end.
static int timing_close(Event *ev, int from, hipStream_t st) { return ev ? timing_record(ev, from, EV_END, st) : TSX_HIP_OK; }
// The same, and the tuple is parked in ev_open: its partition phase runs in a later call, which records those events again.
static int timing_close_parked(tsx_hip_map *m, Event *ev, int from, hipStream_t st) {
    TSX_TRY(timing_close(ev, from, st));
    if (ev) m->ev_open.push_back((long)(ev - m->ev.data()));
    return TSX_HIP_OK;
}
// The oldest parked tuple, or null: timing off, none parked, or parked before the tuples were reset.
static Event *timing_parked(tsx_hip_map *m) {
    if (!m->timing || m->ev_open.empty() || (size_t)m->ev_open.front() + EV_N > m->ev_used) return nullptr;
    return &m->ev[(size_t)m->ev_open.front()];
}
// ... taken off the list (a stale one is dropped as well).
static Event *timing_take_parked(tsx_hip_map *m) {
    Event *ev = timing_parked(m);
    if (!m->ev_open.empty()) m->ev_open.pop_front();
    return ev;
}

// The first walk of a sharded step: what its tuple counts as level 1 starts here (the walks, up to the start of level 2).
static int timing_walks_begin(tsx_hip_map *m, hipStream_t st) {
    Event *ev = timing_parked(m);
    if (ev) { TSX_TRY(timing_record(ev, EV_PART, EV_PART, st)); m->sh_ev3 = true; }
    return TSX_HIP_OK;
}

// ---- one text piece on the device: line pass, then describe / count / scan -------------------------------------------------
struct PieceText { const uint8_t *text; uint64_t n, own_end; int head_open; uint64_t ntiles; };

// The line pass (tile line ends, then their exclusive scan from *d_carry) over the start positions [0, own_end) of
// d_text (n readable bytes).
static int line_pass(tsx_hip_map *m, const uint8_t *d_text, uint64_t n, uint64_t own_end, int head_open, hipStream_t st) {
    const uint64_t ntiles = (own_end + TILE - 1) / TILE;
    TSX_TRY(ensure_tiles(m, ntiles, st));
    const int g1 = (int)std::min<uint64_t>(ntiles, (uint64_t)m->cus * 8);
    hipLaunchKernelGGL(line_count_kernel, dim3(g1), dim3(NT), 0, st, d_text, n, own_end, head_open, m->d_tile.get(), ntiles);
    const uint64_t nchunks = (ntiles + SCAN_CHUNK - 1) / SCAN_CHUNK;
    uint32_t *chunk = m->d_tile.get() + m->tile_cap;
    hipLaunchKernelGGL(line_chunk_sum_kernel, dim3((uint32_t)nchunks), dim3(SCAN_CHUNK), 0, st, (const uint32_t *)m->d_tile.get(),
                       ntiles, chunk);
    hipLaunchKernelGGL(line_chunk_scan_kernel, dim3(1), dim3(1024), 0, st, chunk, nchunks, m->d_carry.get());
    hipLaunchKernelGGL(line_scan_kernel, dim3((uint32_t)nchunks), dim3(SCAN_CHUNK), 0, st, m->d_tile.get(), ntiles,
                       (const uint32_t *)chunk);
    HIP_TRY(hipGetLastError());
    return TSX_HIP_OK;
}

// strip_desc_kernel without a homopolymer output: `grid` workgroups describe the piece, one region of desc_cap per wave.
static void launch_strip_desc(tsx_hip_map *m, int grid, hipStream_t st, const TableParams &pp, const PieceText &t, uint4 *desc,
                              uint64_t desc_cap, unsigned long long *desc_cnt, unsigned long long *kmer_sum, int long_desc) {
    DISPATCH_BR(m, hipLaunchKernelGGL((strip_desc_kernel<false, BRV>), dim3(grid), dim3(NT), 0, st, pp, t.text, t.n, t.own_end,
                                      t.head_open, (const uint32_t *)m->d_tile.get(), t.ntiles, desc, desc_cap, desc_cnt, kmer_sum,
                                      long_desc, (unsigned long long *)nullptr, m->qmap_cur));
}

// The piece is only DESCRIBED: packed into dsc.out, or (dsc.owners) left region by region in buffer 1 for mini_split.
// Whatever partitions and builds follows in other calls: the tuple is closed here and parked for them.
static int describe_piece(tsx_hip_map *m, const PieceText &t, const DescOut &dsc, Event *ev, hipStream_t st) {
    const uint64_t ntiles = t.ntiles;
    const int gdd = (int)std::min<uint64_t>(ntiles, (uint64_t)m->cus * 8), gdr = gdd * (NT / 64);
    const uint32_t du = dsc.long_desc ? 2u : 1u;   // 16-byte units per description (long: four strips in 32 bytes)
    const uint64_t dcap = ((ntiles + gdd - 1) / gdd) * (dsc.long_desc ? 16 : 64);
    TSX_TRY(grow(st, m->d_buf[1], (size_t)gdr * dcap * du * 16));
    // region sizes | region offsets | total
    TSX_TRY(grow(st, m->d_desc_cnt, ((size_t)2 * gdr + 16) * 8 + (size_t)MZ_MAX_RANKS * m->cus * MZ_WG_PER_CU * 4 + 64));
    unsigned long long *d_cnt = m->d_desc_cnt.get(), *d_offs = d_cnt + gdr, *d_tot = d_offs + gdr;
    uint4 *regions = (uint4 *)m->d_buf[1].get();
    if (dsc.owners) {   // owner = f(minimizer): the regions stay where they are, mini_split hands them out by owner
        // homopolymers leave here already: counted in the four words behind the chunk counters
        unsigned long long *d_hom = d_cnt + 2 * (size_t)gdr + 8 + ((size_t)MZ_MAX_RANKS * m->cus * MZ_WG_PER_CU + 1) / 2;
        HIP_TRY(hipMemsetAsync(d_hom, 0, 32, st));
        hipLaunchKernelGGL(strip_desc_kernel<true>, dim3(gdd), dim3(NT), 0, st, m->p, t.text, t.n, t.own_end, t.head_open,
                           (const uint32_t *)m->d_tile.get(), ntiles, regions, dcap, d_cnt, dsc.sum, 0, d_hom);
        HIP_TRY(hipGetLastError());
        m->mz_regions = (uint32_t)gdr; m->mz_dcap = dcap;
        return timing_close_parked(m, ev, EV_SCAN_END, st);
    }
    launch_strip_desc(m, gdd, st, m->p, t, regions, dcap, d_cnt, dsc.sum, dsc.long_desc);
    hipLaunchKernelGGL(desc_prefix_kernel, dim3(1), dim3(1024), 0, st, (const unsigned long long *)d_cnt, (uint32_t)gdr,
                       d_offs, d_tot, dcap, (uint64_t)dsc.cap, m->p.stats);
    hipLaunchKernelGGL(desc_pack_kernel, dim3(std::min(gdr, m->cus * 8)), dim3(256), 0, st, (const uint4 *)regions, dcap,
                       (const unsigned long long *)d_cnt, (const unsigned long long *)d_offs, (uint32_t)gdr, dsc.out,
                       dsc.cap * du, du);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(dsc.count, d_tot, 8, hipMemcpyDeviceToDevice, st));
    return timing_close_parked(m, ev, EV_SCAN_END, st);
}

// The atomic path: count_fastq_kernel inserts every k-mer where it finds it (an armed prefilter is consulted here alone).
static int count_piece_atomic(tsx_hip_map *m, const PieceText &t, Event *ev, hipStream_t st) {
    TSX_TRY(ensure_zeroed(m, st));
    const size_t lut_bytes = m->lut.size() * 8;
    const int g3 = (int)std::min<uint64_t>(t.ntiles, (uint64_t)m->cus * 3);
    if (m->pf_armed) {
        DISPATCH_BR(m, DISPATCH_CANON(m, DISPATCH_WK(m, hipLaunchKernelGGL((count_fastq_kernel<WKV, CANV, BRV, true>), dim3(g3), dim3(NT),
                                                            lut_bytes, st, m->p, t.text, t.n, t.own_end, t.head_open,
                                                            (const uint32_t *)m->d_tile.get(), t.ntiles, m->qmap_cur, m->pf_view()))));
    } else {
        DISPATCH_BR(m, DISPATCH_CANON(m, DISPATCH_WK(m, hipLaunchKernelGGL((count_fastq_kernel<WKV, CANV, BRV>), dim3(g3), dim3(NT),
                                                            lut_bytes, st, m->p, t.text, t.n, t.own_end, t.head_open,
                                                            (const uint32_t *)m->d_tile.get(), t.ntiles, m->qmap_cur))));
    }
    HIP_TRY(hipGetLastError());
    return timing_close(ev, EV_SCAN_END, st);
}

// The scan fused with radix level 1 (local runs, one-limb keys, two radix levels), in two kernels: strip descriptions
// (16 B per strip with a k-mer start, one region per wave, in buffer 0 -- level 2 overwrites it later), then the walk with
// every lane busy.  All keys stay on this GPU: a ring flush per quarter strip (flush_q = 1).
static int scan_fused(tsx_hip_map *m, const PieceText &t, PartPlan &pl, const TableParams &pp, int gd, hipStream_t st) {
    const int gdreg = gd * (NT / 64);
    const uint32_t nq2 = pl.nb1 * pl.cpr2;
    TSX_TRY(ensure_ovq(m, (size_t)nq2 + pl.G1, pl.rw, st));
    // (TSX_HIP_LOCAL_LONG=1: four strips per 32-byte description, as in the exchange of a sharded run)
    const char *ll_env = getenv("TSX_HIP_LOCAL_LONG");
    const int lng = ll_env ? (atoi(ll_env) != 0) : 0;
    const uint64_t desc_cap = ((t.ntiles + gd - 1) / gd) * (lng ? 16 : 64);
    TSX_TRY(grow(st, m->d_buf[0], (size_t)gdreg * desc_cap * (lng ? 32 : 16)));
    launch_strip_desc(m, gd, st, pp, t, (uint4 *)m->d_buf[0].get(), desc_cap, pl.c_log, nullptr, lng);
    HIP_TRY(hipGetLastError());
    WalkPartLaunch w;
    w.grid = pl.G1;
    w.desc = (const uint4 *)m->d_buf[0].get(); w.desc_cap = desc_cap; w.desc_cnt = pl.c_log; w.nregions = (uint32_t)gdreg;
    w.dst = pl.buf1; w.dst_cap = pl.cap1; w.dst_cnt = pl.c_l1;
    w.nb = pl.nb1; w.shift = (uint32_t)(m->p.l - pl.b1);
    w.ovq_all = m->d_ovq.get() + (size_t)nq2 * OVQ_CAP; w.ovq_cnt = m->d_ovq_cnt.get() + nq2; w.ovq_cap = OVQ_CAP;
    w.dst_gtot = pl.G1; w.long_desc = lng; w.flush_q = 1u;
    launch_walk_part(m, st, pp, w);
    pl.l1_wgm = w.dst_wgm != 0;   // level 2 and the skew probe read the lists in the order the walk left them
    m->l1_seen = L1Seen{(size_t)(pl.c_l1 - m->d_cnt.get()), pl.nb1, pl.G1, pl.cpr2, pl.cap1, w.dst_wgm};
    return TSX_HIP_OK;
}

// The key log form (sharded scans, one-level tables, multi-limb keys), in two kernels as well: descriptions into buffer 1
// (level 1 fills it only afterwards; multi-limb: first k-mer + entering bases + validity), then the walk with every lane
// busy into the wave's log region, with the histogram by level-1 bucket -- or by owner GPU for a sharded scan.
static int scan_key_log(tsx_hip_map *m, const PieceText &t, PartPlan &pl, const TableParams &pp, int gs, int gd,
                        uint32_t hist_nb, uint32_t hist_shift, hipStream_t st) {
    const int wk = m->p.wk, gdreg = gd * (NT / 64);
    const int du = (2 * wk + 2 + 3) / 4;   // 16-byte units per description (one-limb keys: 1)
    const uint64_t desc_cap = ((t.ntiles + gd - 1) / gd) * 64;
    TSX_TRY(grow(st, m->d_buf[1], (size_t)gdreg * desc_cap * du * 16));
    pl.buf1 = m->d_buf[1].get();
    TSX_TRY(grow(st, m->d_desc_cnt, (size_t)gdreg * 8));
    uint4 *regions = (uint4 *)m->d_buf[1].get();
#define TSX_DESC_WIDE(WKV)                                                                                                     \
    DISPATCH_BR(m, hipLaunchKernelGGL((strip_desc_wide_kernel<WKV, BRV>), dim3(gd), dim3(NT), 0, st, pp, t.text, t.n, t.own_end, \
                                      t.head_open, (const uint32_t *)m->d_tile.get(), t.ntiles, regions, desc_cap,            \
                                      m->d_desc_cnt.get(), m->qmap_cur))
    switch (wk) {
        case 1:
            launch_strip_desc(m, gd, st, pp, t, regions, desc_cap, m->d_desc_cnt.get(), nullptr, 0);
            HIP_TRY(hipGetLastError());
            break;
        case 2: TSX_DESC_WIDE(2); break;
        case 3: TSX_DESC_WIDE(3); break;
        default: TSX_DESC_WIDE(4); break;
    }
#undef TSX_DESC_WIDE
    WalkLogLaunch w;
    w.grid = (uint32_t)gs;
    w.desc = regions; w.desc_cap = desc_cap; w.desc_cnt = m->d_desc_cnt.get(); w.nregions = (uint32_t)gdreg;
    w.log = m->d_buf[0].get(); w.log_cap = pl.log_cap; w.log_cnt = pl.c_log;
    w.hist = pl.d_hist; w.hist_nb = hist_nb; w.hist_shift = hist_shift;
    launch_walk_log(m, st, pp, w);
    return TSX_HIP_OK;
}

// Sharded scan, level 0: every log region split by owner into the caller's send buffer (exact offsets).
static int split_by_owner(tsx_hip_map *m, const PartPlan &pl, int greg, uint32_t nown, const ShardOut &sh, hipStream_t st) {
    if ((uint64_t)greg * pl.log_cap > sh.send_cap || (sh.own && (uint64_t)greg * pl.log_cap > sh.own_cap)) return TSX_HIP_ERANGE;
    hipLaunchKernelGGL(offsets_rows_kernel, dim3(nown), dim3(1024), 0, st, (const uint32_t *)pl.d_hist, pl.d_offs,
                       (uint32_t)greg, pl.c_bcnt);
    hipLaunchKernelGGL(offsets_finish_kernel, dim3(1), dim3(1024), 0, st, nown, pl.c_bstart, pl.c_bcnt);
    hipLaunchKernelGGL(split_owner_kernel, dim3(std::min(greg, m->cus * 8)), dim3(PART_NT), 0, st,
                       (const uint64_t *)m->d_buf[0].get(), (const unsigned long long *)pl.c_log, pl.log_cap,
                       (uint32_t)greg, sh.send, (const unsigned long long *)pl.d_offs,
                       (const unsigned long long *)pl.c_bstart, (const unsigned long long *)pl.c_bcnt, nown,
                       (uint32_t)m->p.l, sh.own, m->p.shard, sh.key_sum);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(sh.counts, pl.c_bcnt, nown * sizeof(unsigned long long), hipMemcpyDeviceToDevice, st));
    return TSX_HIP_OK;
}

// The partitioned path: scan into level-1 sub-lists or a key log, then level 1 / level 2 / build -- or, for a sharded scan
// (sh.send), the split by owner: hot keys go to `hot`, and the partition phase follows in tsx_hip_shard_build_device.
static int count_piece_partitioned(tsx_hip_map *m, const PieceText &t, const ShardOut &sh, const HotOut &hot, Event *ev,
                                   hipStream_t st) {
    const TableParams &p = m->p;
    const uint64_t own_end = t.own_end, ntiles = t.ntiles;
    const bool sharded = sh.send != nullptr;
    // FASTQ: the quality line is as long as the sequence, at most half of the bytes start a k-mer; FASTA: all may
    const uint64_t maxrec = (p.line_mask == 3 ? own_end / 2 : own_end) + 65536;
    const uint32_t nown = 1u << (p.lg - p.l);
    // the scan kernels of this path keep one log region per WAVE
    // workgroups per CU of the walk that writes the key log (it carries no tile state): 6 for two-limb keys, 3 above
    // (LUT of up to 32 KiB)
    const int scan_wgs = (p.wk == 1) ? SCAN_WG_PER_CU : (p.wk == 2 ? 6 : 3);
    const int gs = (int)std::min<uint64_t>(ntiles, (uint64_t)m->cus * scan_wgs);
    const int greg = gs * (NT / 64);
    PartPlan pl;
    // The walk fused with radix level 1 (local runs, one-limb keys, two radix levels); TSX_HIP_FUSE=0: the key log +
    // a separate level 1 (what sharded scans and one-level tables take).  Read per call: the tests run both in one process.
    const char *fuse_env = getenv("TSX_HIP_FUSE");
    const int fuse = (fuse_env && atoi(fuse_env) == 0) ? 0 : 2;
    const int g_sp = (int)std::min<uint64_t>((own_end + 8191) / 8192, (uint64_t)m->cus * 2);   // walk workgroups
    // strip_desc_kernel: 52 VGPRs, 2.4 KiB of LDS -- eight workgroups per CU (five: 3.9 ms for both kernels, eight: 3.7)
    const int desc_wgs = 8;
    const int gd = (int)std::min<uint64_t>(ntiles, (uint64_t)m->cus * desc_wgs), gdreg = gd * (NT / 64);
    const bool want_fuse = fuse && !sharded && p.wk == 1;

    int rc = plan_partition(m, maxrec, (want_fuse && fuse == 2) ? std::max(greg, gdreg) : greg, true, sharded ? nown : 0, st,
                            pl, want_fuse ? g_sp : 0);
    if (rc == TSX_HIP_OK && want_fuse && !pl.fused)   // a one-level table: the key log form, planned for its own regions
        rc = plan_partition(m, maxrec, greg, true, 0, st, pl, 0);
    if (rc != TSX_HIP_OK) return rc;
    // what cannot take the fast route: the caller's hot list (sharded scan), else the map's deferred list
    TableParams pp = m->p;
    if (sharded) {
        pp.defer = DeferList{hot.keys, hot.cnts, hot.n, hot.cap};
    } else {
        TSX_TRY(ensure_deferred(m, maxrec, st));
        HIP_TRY(hipMemsetAsync(m->d_def_n.get(), 0, 8, st));
        pp.defer = m->defer();
    }
    if (pl.fused) { TSX_TRY(scan_fused(m, t, pl, pp, gd, st)); }
    else { TSX_TRY(scan_key_log(m, t, pl, pp, gs, gd, sharded ? nown : pl.nb1, (uint32_t)(sharded ? p.l : p.l - pl.b1), st)); }
    HIP_TRY(hipGetLastError());
    if (ev) TSX_TRY(timing_record(ev, EV_SCAN_END, EV_PART, st));
    if (sharded) {
        TSX_TRY(split_by_owner(m, pl, greg, nown, sh, st));
        return timing_close_parked(m, ev, EV_PART, st);   // (tsx_hip_shard_build_device records the partition phase again)
    }
    TSX_TRY(run_partition_build(m, pl, m->d_buf[0].get(), nullptr, pl.log_cap, st, ev));
    return timing_close(ev, EV_END, st);
}

// One FASTQ piece already on the device: the line pass, then one of the above.
static int run_fastq_piece(tsx_hip_map *m, const uint8_t *d_text, uint64_t n, uint64_t own_end, int head_open,
                           hipStream_t st, ShardOut sh = ShardOut(), HotOut hot = HotOut(), DescOut dsc = DescOut()) {
    if (own_end == 0) return TSX_HIP_OK;
    const bool describe = dsc.out || dsc.owners;
    // (the counting entry points refuse these before they queue anything: prefilter_count_ok)
    if (m->pf_armed && (sh.send || describe)) return TSX_HIP_EINVAL;
    const PieceText t{d_text, n, own_end, head_open, (own_end + TILE - 1) / TILE};
    TSX_TRY(ensure_tiles(m, t.ntiles, st));   // (before the tuple opens: its first event lies behind a reallocation)
    Event *ev = nullptr;
    TSX_TRY(timing_open(m, ev, st));
    TSX_TRY(line_pass(m, d_text, n, own_end, head_open, st));
    if (ev) TSX_TRY(timing_record(ev, EV_SCAN, EV_SCAN, st));
    if (describe) return describe_piece(m, t, dsc, ev, st);
    // Which insert path?  The partitioned path rewrites every touched segment once (2 x table bytes at worst), the atomic
    // path pays ~60 ps per k-mer.  (A table built slab by slab takes its partitioned path in count_slabs, over the whole
    // text at once.)  An armed prefilter: the atomic path whatever the ratio of text to table (the partitioned walk does
    // not consult B).
    const bool use_part = !m->pf_armed && (sh.send || (can_partition(m) && !slab_bits(m) &&
                                         (m->path == 2 || (m->path == 0 && own_end * 32 >= m->lay.table_bytes))));
    return use_part ? count_piece_partitioned(m, t, sh, hot, ev, st) : count_piece_atomic(m, t, ev, st);
}

// The common opening of the device entry points of the exchanges (tsx_hip_shard_* / tsx_hip_mini_*): canonical tables
// and tables with a base rule are refused, the map counts as used, then the entry point's own argument tests
// (`args_rc`: a callable that returns their code, run only on a map that exists), then the device and the stream.
template <class ArgTests>
static int exch_entry(tsx_hip_map *m, void *stream, hipStream_t &st, ArgTests args_rc) {
    if (exch_refused(m)) return TSX_HIP_EINVAL;   // canonical / base rule: single-table and merge paths only
    if (!m) return TSX_HIP_EINVAL;
    m->used = true;
    TSX_TRY(args_rc());
    HIP_TRY(hipSetDevice(m->device));
    st = pick_stream(m, stream);
    return TSX_HIP_OK;
}

extern "C" int tsx_hip_shard_scan_window_device(tsx_hip_map *m, const void *dev_text, size_t n_total, size_t win_off,
                                                size_t win_len, void *dev_send, size_t send_cap_keys, void *dev_own,
                                                size_t own_cap_keys, void *dev_send_counts, void *dev_hot_keys,
                                                void *dev_hot_counts, size_t hot_cap, void *dev_hot_n,
                                                void *dev_key_sum, void *stream) {
    hipStream_t st;
    TSX_TRY(exch_entry(m, stream, st, [&]() -> int {
        if ((!dev_text && n_total) || ((uintptr_t)dev_text & 15) || (win_off & 15) || !dev_send || !dev_send_counts ||
            !dev_hot_keys || !dev_hot_counts || !dev_hot_n || win_off > n_total || win_len > n_total - win_off)
            return TSX_HIP_EINVAL;
        if (m->p.wk != 1 || m->p.W != 1) return TSX_HIP_EINVAL;  // one-limb keys only (k <= 32)
        return win_len >= ((size_t)4 << 30) ? TSX_HIP_ERANGE : TSX_HIP_OK;  // one window per call
    }));
    if (win_off == 0) HIP_TRY(hipMemsetAsync(m->d_carry.get(), 0, 64, st));   // line index restarts with the text
    HIP_TRY(hipMemsetAsync(dev_hot_n, 0, 8, st));
    HIP_TRY(hipMemsetAsync(dev_send_counts, 0, sizeof(unsigned long long) << (m->p.lg - m->p.l), st));
    if (win_len == 0) return TSX_HIP_OK;
    HotOut hot;
    hot.keys = (uint64_t *)dev_hot_keys; hot.cnts = (uint64_t *)dev_hot_counts; hot.cap = hot_cap;
    hot.n = (unsigned long long *)dev_hot_n;
    ShardOut sh;
    sh.send = (uint64_t *)dev_send; sh.send_cap = send_cap_keys;
    sh.own = (uint64_t *)dev_own; sh.own_cap = own_cap_keys;
    sh.counts = (unsigned long long *)dev_send_counts; sh.key_sum = (unsigned long long *)dev_key_sum;
    // the window owns win_len start positions and sees the k-1 bytes after them; whether it starts inside a
    // line is read from the byte in front of it, on the device
    const size_t halo = (size_t)m->p.k - 1;
    const size_t len = std::min(win_len + halo, n_total - win_off);
    return run_fastq_piece(m, (const uint8_t *)dev_text + win_off, len, win_len, win_off ? -1 : 0, st, sh, hot);
}

extern "C" int tsx_hip_shard_scan_device(tsx_hip_map *m, const void *dev_text, size_t n, void *dev_send,
                                         size_t send_cap_keys, void *dev_send_counts, void *dev_hot_keys,
                                         void *dev_hot_counts, size_t hot_cap, void *dev_hot_n, void *stream) {
    if (exch_refused(m)) return TSX_HIP_EINVAL;   // canonical / base rule: single-table and merge paths only
    if (m) m->used = true;
    return tsx_hip_shard_scan_window_device(m, dev_text, n, 0, n, dev_send, send_cap_keys, nullptr, 0, dev_send_counts,
                                            dev_hot_keys, dev_hot_counts, hot_cap, dev_hot_n, nullptr, stream);
}

extern "C" int tsx_hip_shard_send_capacity(tsx_hip_map *m, size_t text_bytes, size_t *keys_out) {
    if (exch_refused(m)) return TSX_HIP_EINVAL;   // canonical / base rule: single-table and merge paths only
    if (!m || !keys_out) return TSX_HIP_EINVAL;
    const uint64_t ntiles = (text_bytes + TILE - 1) / TILE;
    const int g = (int)std::max<uint64_t>(1, std::min<uint64_t>(ntiles, (uint64_t)m->cus * SCAN_WG_PER_CU)) * (NT / 64);
    const uint64_t maxrec = (m->p.line_mask == 3 ? text_bytes / 2 : text_bytes) + 65536;
    const uint64_t log_cap = (maxrec / g + maxrec / g / 3 + 2048 + 1) & ~1ULL;
    *keys_out = (size_t)g * log_cap;
    return TSX_HIP_OK;
}

extern "C" int tsx_hip_shard_build_pieces_device(tsx_hip_map *m, const void *dev_keys, const uint64_t *piece_off,
                                                 const uint64_t *piece_cnt, size_t npieces, void *dev_key_sum,
                                                 void *stream) {
    if (exch_refused(m)) return TSX_HIP_EINVAL;   // canonical / base rule: single-table and merge paths only
    if (m) m->used = true;
    if (!m || !dev_keys || ((uintptr_t)dev_keys & 7) || (npieces && (!piece_off || !piece_cnt))) return TSX_HIP_EINVAL;
    unsigned long long *key_sum = (unsigned long long *)dev_key_sum;
    uint64_t n_keys = 0;
    for (size_t i = 0; i < npieces; ++i) n_keys += piece_cnt[i];
    if (n_keys == 0) return TSX_HIP_OK;
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t st = pick_stream(m, stream);
    const uint64_t *keys = (const uint64_t *)dev_keys;
    if (!can_partition(m)) {  // tiny tables: plain atomic inserts of the hashed keys
        int rcz = ensure_zeroed(m, st);
        if (rcz != TSX_HIP_OK) return rcz;
        for (size_t i = 0; i < npieces; ++i) {
            if (!piece_cnt[i]) continue;
            hipLaunchKernelGGL(add_hashed_kernel, dim3(grid_for(m, piece_cnt[i], 8)), dim3(PART_NT), 0, st, m->p,
                               keys + piece_off[i], (const uint64_t *)nullptr, (uint64_t)piece_cnt[i], key_sum);
            HIP_TRY(hipGetLastError());
        }
        if (!m->ev_open.empty()) m->ev_open.pop_front();
        return TSX_HIP_OK;
    }
    // regions of the level-1 partition: every piece cut into runs of about n_keys / (3 per CU) keys
    const uint64_t want = std::max<uint64_t>(1, std::min<uint64_t>((n_keys + 4095) / 4096, (uint64_t)m->cus * 3));
    const uint64_t region_len = (n_keys + want - 1) / want;
    m->h_regions.clear();
    std::vector<unsigned long long> cnts;
    for (size_t i = 0; i < npieces; ++i)
        for (uint64_t o = 0; o < piece_cnt[i]; o += region_len) {
            m->h_regions.push_back(piece_off[i] + o);
            cnts.push_back(std::min<uint64_t>(region_len, piece_cnt[i] - o));
        }
    const int g = (int)m->h_regions.size();
    m->h_regions.insert(m->h_regions.end(), cnts.begin(), cnts.end());
    PartPlan pl;
    // Level 1 without a histogram pass: every region's workgroup keeps its own fixed-capacity sub-list per bucket
    // (as level 2 does), level 2 reads a bucket as the regions' pieces -- the plan's `fused` form with G1 = regions.
    // (One-level tables, many-limb keys: histogram + exact offsets as before.)
    int rc = plan_partition(m, n_keys + 65536, g, false, 0, st, pl, m->p.wk == 1 ? g : 0);
    if (rc != TSX_HIP_OK) return rc;
    rc = ensure_deferred(m, n_keys + 65536, st);
    if (rc != TSX_HIP_OK) return rc;
    HIP_TRY(hipMemsetAsync(m->d_def_n.get(), 0, 8, st));
    // region table: starts into c_rstart, sizes into c_log (plan_partition laid them out back to back: [c_log | c_rstart])
    HIP_TRY(hipMemcpyAsync(pl.c_rstart, m->h_regions.data(), (size_t)g * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(pl.c_log, m->h_regions.data() + g, (size_t)g * 8, hipMemcpyHostToDevice, st));
    Event *ev = timing_take_parked(m);
    if (ev) TSX_TRY(timing_record(ev, EV_PART, EV_PART, st));   // the histogram of the received keys counts as level 1
    if (pl.fused) {
        TSX_TRY(ensure_ovq(m, (size_t)pl.nb1 * pl.cpr2 + pl.G1, pl.rw, st));
        TableParams pp = m->p;
        pp.defer = m->defer();
        RingLaunch r = recv_level1(m, pl, (uint32_t)g, 0);
        r.src = keys; r.src_start = pl.c_rstart; r.src_cnt = pl.c_log; r.nregions = (uint32_t)g;
        r.key_sum = key_sum; r.dst_nr = (uint32_t)g;
        launch_ring(st, pp, r);
    } else {
        hipLaunchKernelGGL(hist_kernel, dim3(g), dim3(PART_NT), 0, st, keys, (uint32_t)g, pl.nb1, (uint32_t)(m->p.l - pl.b1),
                           pl.d_hist, (const unsigned long long *)pl.c_rstart, (const unsigned long long *)pl.c_log, key_sum);
    }
    HIP_TRY(hipGetLastError());
    TSX_TRY(run_partition_build(m, pl, keys, pl.c_rstart, 0, st, ev));
    return timing_close(ev, EV_END, st);
}

extern "C" int tsx_hip_shard_build_device(tsx_hip_map *m, const void *dev_keys, size_t n_keys, void *dev_key_sum,
                                          void *stream) {
    if (exch_refused(m)) return TSX_HIP_EINVAL;   // canonical / base rule: single-table and merge paths only
    if (m) m->used = true;
    if (!m || (!dev_keys && n_keys)) return TSX_HIP_EINVAL;
    if (n_keys == 0) return TSX_HIP_OK;
    const uint64_t off = 0, cnt = n_keys;
    return tsx_hip_shard_build_pieces_device(m, dev_keys, &off, &cnt, 1, dev_key_sum, stream);
}

// ---- sharded run, level 1 window by window ------------------------------------------------------------------
// The keys of exchange window w are partitioned by level 1 as soon as they have arrived (the exchange of the later
// windows is still running); only level 2 and the build wait for the last window.
static int l1_supported(tsx_hip_map *m) {
    if (!m || !can_partition(m) || m->p.wk != 1 || m->p.W != 1) return 0;
    return radix_bits(m->p.l - m->p.S).b2 > 0 ? 1 : 0;
}

extern "C" int tsx_hip_shard_l1_supported(tsx_hip_map *m) { return exch_refused(m) ? 0 : l1_supported(m); }

extern "C" int tsx_hip_shard_l1_window_device(tsx_hip_map *m, const void *dev_keys, size_t n_keys, uint32_t window,
                                              uint32_t nwindows, size_t est_total_keys, void *dev_key_sum, void *stream) {
    hipStream_t st;
    TSX_TRY(exch_entry(m, stream, st, [&]() -> int {
        if ((!dev_keys && n_keys) || ((uintptr_t)dev_keys & 7) || nwindows == 0 || window >= nwindows) return TSX_HIP_EINVAL;
        return l1_supported(m) ? TSX_HIP_OK : TSX_HIP_EINVAL;
    }));
    // one workgroup per region, two workgroups per CU: every window's launch fills the chip once
    const uint32_t rw0 = (uint32_t)std::min<uint64_t>((uint64_t)m->cus * 2, (uint64_t)PART_MAX_PIECES * level2_cpr(m) / nwindows);
    TSX_TRY(sharded_l1_step(m, window == 0, rw0, nwindows, nwindows, std::max<uint64_t>(est_total_keys, n_keys) + 65536, st));
    PartPlan &pl = *m->sh_pl;
    if (window == 0) m->h_regions.assign((size_t)2 * pl.G1, 0);
    if (n_keys == 0) return TSX_HIP_OK;
    // the window's keys in sh_rw equal runs
    const uint32_t rw = m->sh_rw, g1 = pl.G1;
    const uint64_t len = (n_keys + rw - 1) / rw;
    unsigned long long *hs = m->h_regions.data() + (size_t)window * rw, *hc = m->h_regions.data() + g1 + (size_t)window * rw;
    for (uint32_t r = 0; r < rw; ++r) {
        const uint64_t o = std::min<uint64_t>((uint64_t)r * len, n_keys);
        hs[r] = o;
        hc[r] = std::min<uint64_t>(len, n_keys - o);
    }
    unsigned long long *ds = pl.c_rstart + (size_t)window * rw, *dc = pl.c_log + (size_t)window * rw;
    HIP_TRY(hipMemcpyAsync(ds, hs, (size_t)rw * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dc, hc, (size_t)rw * 8, hipMemcpyHostToDevice, st));
    TableParams pp = m->p;
    pp.defer = m->defer();
    RingLaunch r = recv_level1(m, pl, rw, window * rw);
    r.src = (const uint64_t *)dev_keys; r.src_start = ds; r.src_cnt = dc; r.nregions = rw;
    r.key_sum = (unsigned long long *)dev_key_sum; r.dst_r0 = window * rw; r.dst_nr = g1;
    launch_ring(st, pp, r);
    HIP_TRY(hipGetLastError());
    return TSX_HIP_OK;
}

// ---- sharded run, DESCRIPTION exchange (small world sizes) -------------------------------------------------------
// Keys cost 8 bytes per k-mer occurrence on the wire; a strip description (16 bytes) stands for up to 16 of them.
// Instead of sending every key to its owner, every GPU describes its window (tsx_hip_shard_desc_window_device), the
// descriptions are ALL-GATHERED, and every GPU walks all of them, keeping the keys it owns
// (tsx_hip_shard_walk_device): N x the rolling work, N/8 of the traffic of the key exchange -- a quarter at N = 2.
extern "C" int tsx_hip_shard_desc_capacity(tsx_hip_map *m, size_t text_bytes, int long_desc, size_t *descs_out) {
    if (exch_refused(m)) return TSX_HIP_EINVAL;   // canonical / base rule: single-table and merge paths only
    if (!m || !descs_out) return TSX_HIP_EINVAL;
    // one description per 16 (long: 64) start positions at most; a long one is 32 bytes, a short one 16
    *descs_out = text_bytes / (long_desc ? 64 : 16) + 4096;
    return TSX_HIP_OK;
}

extern "C" int tsx_hip_shard_desc_window_device(tsx_hip_map *m, const void *dev_text, size_t n_total, size_t win_off,
                                                size_t win_len, int long_desc, void *dev_desc, size_t desc_cap,
                                                void *dev_count, void *dev_kmer_sum, void *stream) {
    hipStream_t st;
    TSX_TRY(exch_entry(m, stream, st, [&]() -> int {
        if ((!dev_text && n_total) || ((uintptr_t)dev_text & 15) || (win_off & 15) || !dev_desc || ((uintptr_t)dev_desc & 15) ||
            !dev_count || win_off > n_total || win_len > n_total - win_off)
            return TSX_HIP_EINVAL;
        if (!l1_supported(m)) return TSX_HIP_EINVAL;
        if (win_len >= ((size_t)4 << 30)) return TSX_HIP_ERANGE;
        return desc_cap < win_len / (long_desc ? 64 : 16) + 1 ? TSX_HIP_ERANGE : TSX_HIP_OK;
    }));
    if (win_off == 0) HIP_TRY(hipMemsetAsync(m->d_carry.get(), 0, 64, st));
    HIP_TRY(hipMemsetAsync(dev_count, 0, 8, st));
    if (win_len == 0) return TSX_HIP_OK;
    DescOut dsc;
    dsc.out = (uint4 *)dev_desc; dsc.cap = desc_cap; dsc.count = (unsigned long long *)dev_count;
    dsc.sum = (unsigned long long *)dev_kmer_sum;
    dsc.long_desc = long_desc ? 1 : 0;
    const size_t halo = (size_t)m->p.k - 1;
    const size_t len = std::min(win_len + halo, n_total - win_off);
    return run_fastq_piece(m, (const uint8_t *)dev_text + win_off, len, win_len, win_off ? -1 : 0, st, ShardOut(), HotOut(), dsc);
}

// ---- owner = f(minimizer) (tsx_minimizer.h): every GPU holds a whole table of the k-mers it owns -------------------
// tsx_hip_mini_window_device describes one text window and splits the descriptions by owner GPU; the caller ships list o
// to GPU o (all-to-all), walks what it received with tsx_hip_shard_walk_device (a map with shard_bits = 0 keeps every key),
// builds with tsx_hip_shard_build_l1_device and adds the homopolymer totals it owns (tsx_hip_add_kmers_device).
extern "C" int tsx_hip_mini_supported(tsx_hip_map *m) {
    return (m && tsx_hip_shard_l1_supported(m) && m->p.lg == m->p.l && mz_supported((uint32_t)m->p.k)) ? 1 : 0;
}

// descriptions one owner's list may take when a text of text_bytes is described at once and split in nparts shares: a
// strip of 16 start positions yields at most one description per owner, + one for a run it shares with its neighbour; a
// region's share rounds up; every workgroup may leave a chunk open, and a list is as long as its busiest workgroup made it
static size_t mini_part_cap(const tsx_hip_map *m, size_t text_bytes, uint32_t nparts) {
    return text_bytes / 8 / nparts + 65536 + 4096 + (size_t)2 * MZ_CHUNK * (size_t)m->cus * MZ_WG_PER_CU;
}
extern "C" int tsx_hip_mini_part_capacity(tsx_hip_map *m, size_t text_bytes, uint32_t nparts, size_t *descs_per_owner_out) {
    if (exch_refused(m)) return TSX_HIP_EINVAL;   // canonical / base rule: single-table and merge paths only
    if (!m || !descs_per_owner_out || nparts == 0) return TSX_HIP_EINVAL;
    *descs_per_owner_out = mini_part_cap(m, text_bytes, nparts);
    return TSX_HIP_OK;
}
extern "C" int tsx_hip_mini_capacity(tsx_hip_map *m, size_t text_bytes, int nranks, size_t *descs_per_owner_out) {
    if (exch_refused(m)) return TSX_HIP_EINVAL;   // canonical / base rule: single-table and merge paths only
    if (!m || !descs_per_owner_out || nranks < 1 || nranks > MZ_MAX_RANKS) return TSX_HIP_EINVAL;
    *descs_per_owner_out = mini_part_cap(m, text_bytes, 1);
    return TSX_HIP_OK;
}

// share `part` of `nparts` of the described text -> one packed list per owner
static int mini_split(tsx_hip_map *m, uint32_t part, uint32_t nparts, int nranks, void *dev_desc, size_t cap_per_owner,
                      void *dev_counts, hipStream_t st) {
    HIP_TRY(hipMemsetAsync(dev_counts, 0, ((size_t)nranks + 4) * 8, st));
    if (m->mz_regions == 0) return TSX_HIP_OK;   // an empty text
    const int gdr = (int)m->mz_regions, gsp = std::min(gdr, m->cus * MZ_WG_PER_CU);
    unsigned long long *d_cnt = m->d_desc_cnt.get(), *count = (unsigned long long *)dev_counts;
    uint32_t *d_used = (uint32_t *)(d_cnt + 2 * (size_t)gdr + 8);   // chunks taken per (owner, workgroup)
    hipLaunchKernelGGL(desc_owner_split_kernel, dim3(gsp), dim3(MZ_NT), 0, st, m->p, (const uint4 *)m->d_buf[1].get(), m->mz_dcap,
                       (const unsigned long long *)d_cnt, (uint32_t)gdr, (uint32_t)nranks, (uint4 *)dev_desc, (uint64_t)cap_per_owner,
                       d_used, count + nranks, part, nparts,
                       (const unsigned long long *)(d_cnt + 2 * (size_t)gdr + 8 + ((size_t)MZ_MAX_RANKS * m->cus * MZ_WG_PER_CU + 1) / 2));
    hipLaunchKernelGGL(desc_owner_finish_kernel, dim3(nranks), dim3(MZ_NT), 0, st, (const uint32_t *)d_used, (uint32_t)gsp,
                       (uint32_t)nranks, (uint4 *)dev_desc, (uint64_t)cap_per_owner, count, m->p.stats);
    HIP_TRY(hipGetLastError());
    return TSX_HIP_OK;
}

static int mini_describe(tsx_hip_map *m, const void *dev_text, size_t n_total, size_t off, size_t len, void *dev_kmer_sum,
                         hipStream_t st) {
    if (off == 0) HIP_TRY(hipMemsetAsync(m->d_carry.get(), 0, 64, st));
    m->mz_regions = 0; m->mz_len = len;
    if (len == 0) return TSX_HIP_OK;
    DescOut dsc;
    dsc.sum = (unsigned long long *)dev_kmer_sum;
    dsc.owners = 1;
    const size_t halo = (size_t)m->p.k - 1;
    const size_t ext = std::min(len + halo, n_total - off);
    return run_fastq_piece(m, (const uint8_t *)dev_text + off, ext, len, off ? -1 : 0, st, ShardOut(), HotOut(), dsc);
}

extern "C" int tsx_hip_mini_describe_device(tsx_hip_map *m, const void *dev_text, size_t n_total, size_t off, size_t len,
                                            void *dev_kmer_sum, void *stream) {
    hipStream_t st;
    TSX_TRY(exch_entry(m, stream, st, [&]() -> int {
        if ((!dev_text && n_total) || ((uintptr_t)dev_text & 15) || (off & 15) || off > n_total || len > n_total - off)
            return TSX_HIP_EINVAL;
        if (!tsx_hip_mini_supported(m)) return TSX_HIP_EINVAL;
        return len >= ((size_t)4 << 30) ? TSX_HIP_ERANGE : TSX_HIP_OK;
    }));
    return mini_describe(m, dev_text, n_total, off, len, dev_kmer_sum, st);
}

extern "C" int tsx_hip_mini_split_device(tsx_hip_map *m, uint32_t part, uint32_t nparts, int nranks, void *dev_desc,
                                         size_t cap_per_owner, void *dev_counts, void *stream) {
    hipStream_t st;
    TSX_TRY(exch_entry(m, stream, st, [&]() -> int {
        if (nparts == 0 || part >= nparts || !dev_desc || ((uintptr_t)dev_desc & 15) || !dev_counts || nranks < 1 ||
            nranks > MZ_MAX_RANKS)
            return TSX_HIP_EINVAL;
        if (!tsx_hip_mini_supported(m)) return TSX_HIP_EINVAL;
        return (m->mz_regions && cap_per_owner < mini_part_cap(m, m->mz_len, nparts)) ? TSX_HIP_ERANGE : TSX_HIP_OK;
    }));
    return mini_split(m, part, nparts, nranks, dev_desc, cap_per_owner, dev_counts, st);
}

extern "C" int tsx_hip_mini_window_device(tsx_hip_map *m, const void *dev_text, size_t n_total, size_t win_off, size_t win_len,
                                          int nranks, void *dev_desc, size_t cap_per_owner, void *dev_counts,
                                          void *dev_kmer_sum, void *stream) {
    hipStream_t st;
    TSX_TRY(exch_entry(m, stream, st, [&]() -> int {
        if ((!dev_text && n_total) || ((uintptr_t)dev_text & 15) || (win_off & 15) || !dev_desc || ((uintptr_t)dev_desc & 15) ||
            !dev_counts || win_off > n_total || win_len > n_total - win_off || nranks < 1 || nranks > MZ_MAX_RANKS)
            return TSX_HIP_EINVAL;
        if (!tsx_hip_mini_supported(m)) return TSX_HIP_EINVAL;
        if (win_len >= ((size_t)4 << 30)) return TSX_HIP_ERANGE;
        size_t need = 0;
        tsx_hip_mini_capacity(m, win_len, nranks, &need);
        return cap_per_owner < need ? TSX_HIP_ERANGE : TSX_HIP_OK;
    }));
    int rc = mini_describe(m, dev_text, n_total, win_off, win_len, dev_kmer_sum, st);
    if (rc != TSX_HIP_OK) return rc;
    return mini_split(m, 0, 1, nranks, dev_desc, cap_per_owner, dev_counts, st);
}

extern "C" int tsx_hip_mini_owner_host(int k, int nranks, const uint64_t *kmers, size_t n, uint32_t *owners_out) {
    if (!mz_supported((uint32_t)k) || nranks < 1 || nranks > MZ_MAX_RANKS || (!kmers && n) || (!owners_out && n)) return TSX_HIP_EINVAL;
    for (size_t i = 0; i < n; ++i) owners_out[i] = mz_owner_of_kmer(kmers[i], (uint32_t)k, (uint32_t)nranks);
    return TSX_HIP_OK;
}

// Walks n_desc packed descriptions (any GPU's), keeps the keys this shard owns and partitions them by radix level 1
// into list set `slot` of `nslots` (slot 0 plans for est_total_keys owned keys in all).  dev_emit_sum += k-mer
// occurrences kept.  Then tsx_hip_shard_build_l1_device.
// tsx_hip_shard_walk_device, and the walks of a table built slab by slab (count_slabs), canonical ones included
static int shard_walk(tsx_hip_map *m, const void *dev_desc, size_t n_desc, int long_desc, uint32_t slot, uint32_t nslots,
                      size_t est_total_keys, void *dev_emit_sum, void *stream) {
    if (!m || (!dev_desc && n_desc) || ((uintptr_t)dev_desc & 15) || nslots == 0 || slot >= nslots) return TSX_HIP_EINVAL;
    if (!l1_supported(m)) return TSX_HIP_EINVAL;
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t st = pick_stream(m, stream);
    // long_desc & 2: what the minimizer exchange sent to a map with shard_bits = 0 -- every key stays, homopolymers were
    // taken out by the sender, about half of a description's 16 positions are valid (a flush every second quarter), and
    // the windows of a step APPEND to one set of level-1 sub-lists (level 2 then reads as many pieces as on one GPU)
    const bool mini = (long_desc & 2) != 0;
    long_desc &= 1;
    if (mini && m->p.lg != m->p.l) return TSX_HIP_EINVAL;
    const uint32_t caller_slots = nslots, caller_slot = slot;
    if (mini) { nslots = 1; slot = 0; }
    const bool first = caller_slot == 0;
    TSX_TRY(sharded_l1_step(m, first, first ? shard_lists_per_slot(m, nslots) : 0, nslots, caller_slots, est_total_keys + 65536, st));
    const PartPlan &pl = *m->sh_pl;
    if (first) TSX_TRY(timing_walks_begin(m, st));
    if (n_desc == 0) return TSX_HIP_OK;
    const uint32_t gw = m->sh_rw;
    const uint64_t chunk = (n_desc + gw - 1) / gw;   // descriptions per workgroup
    // this GPU keeps one key in 2^shard_bits: a ring flush every 1, 2 or 4 quarter strips (walk_part_kernel); every 2
    // in the minimizer exchange
    const uint32_t nown = 1u << (m->p.lg - m->p.l);
    const uint32_t flush_q = mini ? 2u : (nown >= 4 ? 4u : (nown == 2 ? 2u : 1u));
    const int own_mode = mini ? (2 | (caller_slot > 0 ? 4 : 0)) : 1;
    TableParams pp = m->p;
    pp.defer = m->defer();
    // (a canonical map gets here only from count_slabs: the exchanges refuse it)
    WalkPartLaunch w;
    w.grid = gw;
    w.desc = (const uint4 *)dev_desc; w.desc_cap = chunk; w.nregions = gw;
    w.dst = pl.buf1; w.dst_cap = pl.cap1; w.dst_cnt = pl.c_l1;
    w.nb = pl.nb1; w.shift = (uint32_t)(m->p.l - pl.b1);
    const size_t q0 = (size_t)pl.nb1 * pl.cpr2 + (size_t)slot * gw;   // the slot's overflow queues, behind level 2's
    w.ovq_all = m->d_ovq.get() + q0 * OVQ_CAP; w.ovq_cnt = m->d_ovq_cnt.get() + q0; w.ovq_cap = OVQ_CAP;
    w.n_packed = (uint64_t)n_desc; w.dst_g0 = slot * gw; w.dst_gtot = pl.G1; w.own_flags = own_mode;
    w.emit_sum = (unsigned long long *)dev_emit_sum; w.long_desc = long_desc ? 1 : 0; w.flush_q = flush_q;
    launch_walk_part(m, st, pp, w);
    HIP_TRY(hipGetLastError());
    return TSX_HIP_OK;
}

extern "C" int tsx_hip_shard_walk_device(tsx_hip_map *m, const void *dev_desc, size_t n_desc, int long_desc, uint32_t slot,
                                         uint32_t nslots, size_t est_total_keys, void *dev_emit_sum, void *stream) {
    if (exch_refused(m)) return TSX_HIP_EINVAL;   // the exchanges have no canonical form (owners are strand-dependent) nor base rule
    if (m && n_desc) m->used = true;
    return shard_walk(m, dev_desc, n_desc, long_desc, slot, nslots, est_total_keys, dev_emit_sum, stream);
}

// The same in two kernels, for larger world sizes: this GPU keeps one key in N, so the fused walk is mostly waiting
// for its rolling chains at 16 waves per CU (1.9 ms per 1e9 positions at N = 8).  walk_log_kernel in its owner-filtered
// form has no rings to hold (20 waves per CU) and logs the kept keys per wave; level 1 of partition_ring_kernel then
// reads the wave logs as pieces (512 workgroups, each streaming ten of them) into list set `slot` of `nslots`.
extern "C" int tsx_hip_shard_filter_device(tsx_hip_map *m, const void *dev_desc, size_t n_desc, int long_desc, uint32_t slot,
                                           uint32_t nslots, size_t est_total_keys, void *dev_emit_sum, void *stream) {
    hipStream_t st;
    TSX_TRY(exch_entry(m, stream, st, [&]() -> int {
        if ((!dev_desc && n_desc) || ((uintptr_t)dev_desc & 15) || nslots == 0 || slot >= nslots) return TSX_HIP_EINVAL;
        return l1_supported(m) ? TSX_HIP_OK : TSX_HIP_EINVAL;
    }));
    const bool first = slot == 0;
    TSX_TRY(sharded_l1_step(m, first, first ? shard_lists_per_slot(m, nslots) : 0, nslots, nslots, est_total_keys + 65536, st));
    const PartPlan &pl = *m->sh_pl;
    if (first) TSX_TRY(timing_walks_begin(m, st));
    if (n_desc == 0) return TSX_HIP_OK;
    // the wave logs of this slot: the map's own scratch (buffer 0), planned for what this slot may keep
    const int gs = (int)m->cus * SCAN_WG_PER_CU, greg = gs * (NT / 64);
    PartPlan lp;
    const uint64_t keep = est_total_keys / nslots + est_total_keys / nslots / 2 + 65536;
    int rc = plan_partition(m, keep, greg, true, 0, st, lp, 0);
    if (rc != TSX_HIP_OK) return rc;
    TableParams pp = m->p;
    pp.defer = m->defer();
    const uint64_t chunk = (n_desc + greg - 1) / greg;   // descriptions per wave
    WalkLogLaunch w;
    w.grid = (uint32_t)gs;
    w.desc = (const uint4 *)dev_desc; w.desc_cap = chunk; w.nregions = (uint32_t)greg;
    w.log = m->d_buf[0].get(); w.log_cap = lp.log_cap; w.log_cnt = lp.c_log;
    w.hist = lp.d_hist; w.hist_nb = lp.nb1; w.hist_shift = (uint32_t)(m->p.l - lp.b1);
    w.n_packed = (uint64_t)n_desc; w.long_desc = long_desc ? 1 : 0; w.own_only = 1; w.emit_sum = (unsigned long long *)dev_emit_sum;
    launch_walk_log(m, st, pp, w);
    HIP_TRY(hipGetLastError());
    // level 1 reads the wave logs as pieces of ONE region, its gw workgroups sharing them out (cpr), into list set `slot`
    const uint32_t gw = m->sh_rw;
    RingLaunch r = recv_level1(m, pl, gw, slot * gw);
    r.src = m->d_buf[0].get(); r.nregions = 1; r.cpr = gw;
    r.src_pcnt = lp.c_log; r.src_np = (uint32_t)greg; r.src_pcap = lp.log_cap;
    r.dst_r0 = slot; r.dst_nr = nslots;
    launch_ring(st, pp, r);
    HIP_TRY(hipGetLastError());
    return TSX_HIP_OK;
}

// level 2 + build over the sub-lists the windows' level-1 launches have filled
extern "C" int tsx_hip_shard_build_l1_device(tsx_hip_map *m, void *stream) {
    hipStream_t st;
    TSX_TRY(exch_entry(m, stream, st, [&]() -> int { return (!m->sh_pl || !m->sh_pl->fused) ? TSX_HIP_EINVAL : TSX_HIP_OK; }));
    Event *ev = timing_take_parked(m);
    if (ev && !m->sh_ev3) TSX_TRY(timing_record(ev, EV_PART, EV_PART, st));   // (else the first walk of the step has)
    m->sh_ev3 = false;
    TSX_TRY(run_partition_build(m, *m->sh_pl, nullptr, nullptr, 0, st, ev));
    return timing_close(ev, EV_END, st);
}

extern "C" int tsx_hip_add_hashed_device(tsx_hip_map *m, const void *dev_keys, const void *dev_counts, size_t n,
                                         void *stream) {
    if (exch_refused(m)) return TSX_HIP_EINVAL;   // canonical / base rule: single-table and merge paths only
    if (m) m->used = true;
    if (!m || (!dev_keys && n)) return TSX_HIP_EINVAL;
    if (m->p.wk != 1 || m->p.W != 1) return TSX_HIP_EINVAL;
    if (n == 0) return TSX_HIP_OK;
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t st = pick_stream(m, stream);
    int rcz = ensure_zeroed(m, st);
    if (rcz != TSX_HIP_OK) return rcz;
    if (dev_counts) {
        // (key, count) lists are the hot lists of the sharded scan: the same few keys over and over (every scan wave
        // drains its cache).  deferred_insert_kernel sums equal keys of a workgroup's share in LDS first -- one
        // same-address global atomic per workgroup instead of one per entry (0.36 -> 0.04 ms per window's list).
        const int grid = (int)std::min<uint64_t>((uint64_t)m->cus * 2, (n + 511) / 512);
        hipLaunchKernelGGL((deferred_insert_kernel<1>), dim3(grid), dim3(PART_NT), 0, st, m->p, (const uint64_t *)dev_keys,
                           (const uint64_t *)dev_counts, (const unsigned long long *)nullptr, (uint64_t)n, (uint64_t)n);
    } else {
        const int grid = grid_for(m, n, 8);
        hipLaunchKernelGGL(add_hashed_kernel, dim3(grid), dim3(PART_NT), 0, st, m->p, (const uint64_t *)dev_keys,
                           (const uint64_t *)dev_counts, (uint64_t)n, (unsigned long long *)nullptr);
    }
    HIP_TRY(hipGetLastError());
    return TSX_HIP_OK;
}

extern "C" int tsx_hip_set_record_lines(tsx_hip_map *m, int lines) {
    if (!m || (lines != 2 && lines != 4)) return TSX_HIP_EINVAL;
    m->p.line_mask = (uint32_t)lines - 1u;
    return TSX_HIP_OK;
}

extern "C" int tsx_hip_set_path(tsx_hip_map *m, int path) {
    if (!m || path < 0 || path > 2) return TSX_HIP_EINVAL;
    m->path = path;
    return TSX_HIP_OK;
}

extern "C" int tsx_hip_set_timing(tsx_hip_map *m, int enable) {
    if (!m) return TSX_HIP_EINVAL;
    m->timing = enable ? 1 : 0;
    m->ev_used = 0;
    m->ev_open.clear();
    return TSX_HIP_OK;
}

extern "C" int tsx_hip_get_stage_timing(tsx_hip_map *m, double *stage_ms, uint64_t *launches) {
    if (!m) return TSX_HIP_EINVAL;
    HIP_TRY(hipSetDevice(m->device));
    double acc[7] = {0, 0, 0, 0, 0, 0, 0};
    // line, scan, level 1, level 2, build kernel, gap, inserts after the build (overflow queues + deferred list)
    static const struct { TimingEvent from, to; } stage[7] = {
        {EV_BEGIN, EV_SCAN},         {EV_SCAN, EV_SCAN_END}, {EV_PART, EV_L1_END},    {EV_L1_END, EV_L2_END},
        {EV_L2_END, EV_BUILD_END}, {EV_SCAN_END, EV_PART}, {EV_BUILD_END, EV_END}};
    for (size_t i = 0; i + EV_N <= m->ev_used; i += EV_N) {
        HIP_TRY(hipEventSynchronize(m->ev[i + EV_END].get()));
        for (int sgm = 0; sgm < 7; ++sgm) {
            float t = 0;
            HIP_TRY(hipEventElapsedTime(&t, m->ev[i + stage[sgm].from].get(), m->ev[i + stage[sgm].to].get()));
            acc[sgm] += t;
        }
    }
    if (stage_ms) for (int sgm = 0; sgm < 7; ++sgm) stage_ms[sgm] = acc[sgm];
    if (launches) *launches = m->ev_used / EV_N;
    m->ev_used = 0;
    m->ev_open.clear();
    return TSX_HIP_OK;
}

extern "C" int tsx_hip_get_timing(tsx_hip_map *m, double *line_ms, double *count_ms, double *build_ms,
                                  uint64_t *launches) {
    double sgm[7];
    const int rc = tsx_hip_get_stage_timing(m, sgm, launches);
    if (rc != TSX_HIP_OK) return rc;
    if (line_ms) *line_ms = sgm[0];
    if (count_ms) *count_ms = sgm[1];
    if (build_ms) *build_ms = sgm[2] + sgm[3] + sgm[4] + sgm[6];
    return TSX_HIP_OK;
}

// ==== text sources: how a text reaches the device -- host staging, BGZF batches, pieces cut at record boundaries =========

// ---- host staging: two pinned and two device buffers of a piece each -----------------------------------------------------
static int ensure_staging(tsx_hip_map *m, size_t n) {
    const size_t bytes = std::min(m->piece, n) + STAGE_PAD + 128;
    if (m->d_stage[1].cap() >= bytes) return TSX_HIP_OK;   // (allocated last: there when all of them are)
    auto drop = [&] { for (int i = 0; i < 2; ++i) { m->h_stage[i].reset(); m->d_stage[i].reset(); } };
    drop();   // grow: drop the smaller buffers first
    int rc = m->copy_stream.get() ? TSX_HIP_OK : m->copy_stream.create();
    for (int i = 0; i < 2 && rc == TSX_HIP_OK; ++i) {
        if ((rc = m->h_stage[i].alloc(bytes)) == TSX_HIP_OK) rc = m->d_stage[i].alloc(bytes);
        if (rc == TSX_HIP_OK) rc = m->stage_done[i].create();
        if (rc == TSX_HIP_OK) rc = m->stage_in[i].create();
    }
    if (rc != TSX_HIP_OK) drop();   // all four buffers or none
    return rc;
}

// Pageable -> pinned staging copy on several host threads: one thread moves ~10 GB/s,
// the PCIe link ~55 GB/s.  Hardware threads - 2, at least 2 and at most 12.
static void parallel_memcpy(uint8_t *dst, const char *src, size_t len) {
    static const unsigned maxt = [] {   // (initialised once, also when rank threads copy at the same time)
        const unsigned hw = std::thread::hardware_concurrency();
        return std::min(12u, std::max(2u, hw > 2 ? hw - 2 : 2u));
    }();
    const size_t MIN_PER_THREAD = (size_t)8 << 20;
    unsigned nthreads = (unsigned)std::min<size_t>(maxt, len / MIN_PER_THREAD);
    if (nthreads <= 1) { memcpy(dst, src, len); return; }
    std::vector<std::thread> th;
    const size_t per = ((len / nthreads) + 4095) & ~(size_t)4095;
    for (unsigned t = 0; t < nthreads; ++t) {
        const size_t lo = std::min(len, (size_t)t * per), hi = (t + 1 == nthreads) ? len : std::min(len, lo + per);
        if (hi > lo) th.emplace_back([=]() { memcpy(dst + lo, src + lo, hi - lo); });
    }
    for (auto &x : th) x.join();
}

// The piece text[0, len) through h_stage[buf] into d_stage[buf], on stream `st`.  Queued, not waited for.
static int stage_upload(tsx_hip_map *m, int buf, const char *text, size_t len, hipStream_t st) {
    parallel_memcpy(m->h_stage[buf].get(), text, len);
    HIP_TRY(hipMemcpyAsync(m->d_stage[buf].get(), m->h_stage[buf].get(), len, hipMemcpyHostToDevice, st));
    return TSX_HIP_OK;
}

// The driver of the host count calls without a quality rule: the text in pieces that own `piece` start positions and
// carry `halo` more bytes, through the two staging buffers in turn.  Three legs overlap: this piece's host copy, the
// previous piece's H2D copy (its own stream) and the kernels of the piece before that, which
//   per_piece(d_piece, len, own, head_open)      queues on the map's stream (head_open: the piece starts inside a line).
// Waits for the table when the last piece is queued (tsx_hip_sync).
template <class PerPiece>
static int staged_pieces(tsx_hip_map *m, const char *text, size_t n, size_t piece, size_t halo, PerPiece per_piece) {
    TSX_TRY(ensure_staging(m, n));
    hipStream_t st = m->stream.get();
    int buf = 0;
    bool used[2] = {false, false};
    for (size_t off = 0; off < n; off += piece, buf ^= 1) {
        const size_t own = std::min(piece, n - off);
        const size_t len = std::min(own + halo, n - off);
        if (used[buf]) HIP_TRY(hipEventSynchronize(m->stage_done[buf].get()));
        TSX_TRY(stage_upload(m, buf, text + off, len, m->copy_stream.get()));
        HIP_TRY(hipEventRecord(m->stage_in[buf].get(), m->copy_stream.get()));
        HIP_TRY(hipStreamWaitEvent(st, m->stage_in[buf].get(), 0));
        const int head_open = (off > 0 && text[off - 1] != '\n') ? 1 : 0;
        TSX_TRY(per_piece((const uint8_t *)m->d_stage[buf].get(), len, own, head_open));
        HIP_TRY(hipEventRecord(m->stage_done[buf].get(), st));
        used[buf] = true;
    }
    return tsx_hip_sync(m);
}

// ---- blocked gzip (BGZF) input: members found on the host, inflated on the device (tsx_inflate.h) ---------
struct BgzfIndex {
    std::vector<uint64_t> in_off, out_off;
    std::vector<uint32_t> in_len, out_len, crc;
    uint64_t text_bytes = 0;
};
static inline uint32_t le16(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
static inline uint32_t le32(const uint8_t *p) { return le16(p) | (le16(p + 2) << 16); }

// gzip members (RFC 1952) that all carry the BGZF 'BC' extra subfield (SAM specification, section 4.1):
// BSIZE = size of the member - 1.  false: not BGZF (or damaged) -- the caller reads it with zlib instead.
static bool bgzf_index(const uint8_t *gz, size_t n, BgzfIndex &ix) {
    size_t o = 0;
    while (o < n) {
        if (n - o < 18 || gz[o] != 0x1f || gz[o + 1] != 0x8b || gz[o + 2] != 8 || !(gz[o + 3] & 4)) return false;
        if (gz[o + 3] & ~4) return false;   // FNAME/FCOMMENT/FHCRC: not written by bgzip, not parsed here
        const uint32_t xlen = le16(gz + o + 10);
        if (n - o < 12 + (size_t)xlen + 8) return false;
        uint32_t bsize = 0;
        bool found = false;
        for (uint32_t x = 0; x + 4 <= xlen;) {
            const uint8_t *e = gz + o + 12 + x;
            const uint32_t slen = le16(e + 2);
            if (e[0] == 'B' && e[1] == 'C' && slen == 2 && x + 6 <= xlen) { bsize = le16(e + 4); found = true; }
            x += 4 + slen;
        }
        if (!found) return false;
        const size_t total = (size_t)bsize + 1;
        if (total < 12 + (size_t)xlen + 8 || total > n - o) return false;
        const size_t data_off = o + 12 + xlen, data_len = total - (12 + xlen) - 8;
        const uint32_t isize = le32(gz + o + total - 4);
        if (isize > (1u << 16)) return false;   // a BGZF member holds at most 64 KiB
        ix.in_off.push_back(data_off);
        ix.in_len.push_back((uint32_t)data_len);
        ix.out_off.push_back(ix.text_bytes);
        ix.out_len.push_back(isize);
        ix.crc.push_back(le32(gz + o + total - 8));
        ix.text_bytes += isize;
        o += total;
    }
    return !ix.in_off.empty();
}

extern "C" int tsx_hip_bgzf_index_host(const void *gz, size_t n, size_t *members, size_t *text_bytes) {
    if (!gz && n) return TSX_HIP_EINVAL;
    BgzfIndex ix;
    if (!bgzf_index((const uint8_t *)gz, n, ix)) return TSX_HIP_EINVAL;
    if (members) *members = ix.in_off.size();
    if (text_bytes) *text_bytes = (size_t)ix.text_bytes;
    return TSX_HIP_OK;
}

// Device scratch of the BGZF path: the compressed bytes and the member index of ONE batch of members.
struct BgzfDev {
    DevBuf<uint8_t> d_gz, d_ix;
    DevBuf<uint32_t> d_tab;      // CRC-32 tables
};

// Members are inflated in BATCHES of at most this many bytes of text (whole members, at least one), so that a large
// .fastq.gz needs two batch-sized text buffers instead of the whole text at once.  TSX_HIP_BGZF_BATCH: tests.
static size_t bgzf_batch_bytes() {
    // (a launch of the inflate kernel takes as long as ONE member takes, 16 ms, whatever the number of members: few, big batches)
    size_t v = (size_t)3 << 30;
    if (const char *e = getenv("TSX_HIP_BGZF_BATCH")) { const long long x = atoll(e); if (x > 0) v = (size_t)x; }
    return std::max<size_t>(v, (size_t)128 << 10);
}
// The batches of a file, in order: [m0, m1) is the current one -- members from m0 on while the text stays within `batch`
// bytes (or below 4 KiB).  for (BgzfBatches b(ix, batch); !b.done(); b.next()) ...
struct BgzfBatches {
    const BgzfIndex &ix;
    size_t batch, m0 = 0, m1 = 0;
    BgzfBatches(const BgzfIndex &x, size_t bytes) : ix(x), batch(bytes) { m1 = end_from(0); }
    size_t end_from(size_t a) const {
        size_t b = a, acc = 0;
        while (b < ix.in_off.size() && (b == a || acc < 4096 || acc + ix.out_len[b] <= batch)) acc += ix.out_len[b++];
        return b;
    }
    bool done() const { return m0 == ix.in_off.size(); }
    bool first() const { return m0 == 0; }
    bool last() const { return m1 == ix.in_off.size(); }
    size_t text() const { return (size_t)((m1 < ix.out_off.size() ? ix.out_off[m1] : ix.text_bytes) - ix.out_off[m0]); }   // its bytes of text
    void next() { m0 = m1; m1 = end_from(m0); }
    size_t biggest() const {   // the text of the largest batch of the file
        size_t v = 0;
        for (BgzfBatches b(ix, batch); !b.done(); b.next()) v = std::max(v, b.text());
        return v;
    }
};

// Inflates members [m0, m1) of gz: the text of member m0 starts at d_out[0].  Waits for the kernel and checks
// every member's status (stored / fixed / dynamic blocks decoded, ISIZE and CRC-32 right).
static int inflate_batch(const uint8_t *gz, size_t n, const BgzfIndex &ix, size_t m0, size_t m1, BgzfDev &dv,
                         uint8_t *d_out, hipStream_t st) {
    const size_t nm = m1 - m0;
    if (nm == 0) return TSX_HIP_OK;
    // CRC-32 tables for eight bytes per step: crc_tab[j][v] = CRC of byte v followed by j zero bytes
    static uint32_t crc_tab[8 * 256];
    static std::once_flag crc_once;
    std::call_once(crc_once, [] {
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int b = 0; b < 8; ++b) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
            crc_tab[i] = c;
        }
        for (int j = 1; j < 8; ++j)
            for (uint32_t i = 0; i < 256; ++i)
                crc_tab[j * 256 + i] = (crc_tab[(j - 1) * 256 + i] >> 8) ^ crc_tab[crc_tab[(j - 1) * 256 + i] & 0xFFu];
    });
    if (!dv.d_tab.get()) {
        TSX_TRY(dv.d_tab.alloc(sizeof(crc_tab)));
        HIP_TRY(hipMemcpyAsync(dv.d_tab.get(), crc_tab, sizeof(crc_tab), hipMemcpyHostToDevice, st));
        HIP_TRY(hipFuncSetAttribute((const void *)inflate_members_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)INF_LDS_BYTES));
    }
    const size_t lo = (size_t)ix.in_off[m0], hi = (size_t)ix.in_off[m1 - 1] + ix.in_len[m1 - 1];
    const size_t gz_bytes = std::min(n, hi + 16) - lo;       // the bit reader looks up to 16 bytes past a member
    TSX_TRY(grow(st, dv.d_gz, (hi - lo) + 64));
    // one allocation for the index: in_off | out_off | in_len | out_len | crc | status
    TSX_TRY(grow(st, dv.d_ix, nm * (8 + 8 + 4 + 4 + 4 + 4)));
    std::vector<uint64_t> in_off(nm), out_off(nm);
    for (size_t i = 0; i < nm; ++i) { in_off[i] = ix.in_off[m0 + i] - lo; out_off[i] = ix.out_off[m0 + i] - ix.out_off[m0]; }
    uint64_t *d_in_off = (uint64_t *)dv.d_ix.get(), *d_out_off = d_in_off + nm;
    uint32_t *d_in_len = (uint32_t *)(d_out_off + nm), *d_out_len = d_in_len + nm, *d_crc = d_out_len + nm, *d_status = d_crc + nm;
    HIP_TRY(hipMemcpyAsync(dv.d_gz.get(), gz + lo, gz_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_in_off, in_off.data(), nm * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_out_off, out_off.data(), nm * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_in_len, ix.in_len.data() + m0, nm * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_out_len, ix.out_len.data() + m0, nm * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_crc, ix.crc.data() + m0, nm * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(d_status, 0xFF, nm * 4, st));
    hipLaunchKernelGGL(inflate_members_kernel, dim3((uint32_t)((nm + INF_NT - 1) / INF_NT)), dim3(INF_NT), INF_LDS_BYTES, st,
                       (const uint8_t *)dv.d_gz.get(), (const uint64_t *)d_in_off, (const uint32_t *)d_in_len,
                       (const uint64_t *)d_out_off, (const uint32_t *)d_out_len, (const uint32_t *)d_crc, (uint32_t)nm, d_out,
                       d_status, (const uint32_t *)dv.d_tab.get());
    HIP_TRY(hipGetLastError());
    std::vector<uint32_t> status(nm);
    HIP_TRY(hipMemcpyAsync(status.data(), d_status, nm * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));      // (also: in_off / out_off of this frame have been copied)
    for (size_t i = 0; i < nm; ++i)
        if (status[i] != INF_OK) {
            static const char *why[] = {"ok", "deflate data truncated", "reserved block type", "stored block length check",
                                        "bad code lengths", "invalid symbol", "output overrun or distance too far",
                                        "size differs from ISIZE", "CRC-32 mismatch"};
            g_last_error = "BGZF member " + std::to_string(m0 + i) + ": " + (status[i] < 9 ? why[status[i]] : "not decoded");
            return TSX_HIP_EINVAL;
        }
    return TSX_HIP_OK;
}

extern "C" int tsx_hip_inflate_bgzf_host(int device, const void *gz, size_t n, void *out_host, size_t out_cap,
                                         size_t *out_bytes) {
    if ((!gz && n) || !out_bytes) return TSX_HIP_EINVAL;
    BgzfIndex ix;
    if (!bgzf_index((const uint8_t *)gz, n, ix)) { g_last_error = "not a BGZF file (no BC extra field in every gzip member)"; return TSX_HIP_EINVAL; }
    *out_bytes = (size_t)ix.text_bytes;
    if (ix.text_bytes > out_cap || (ix.text_bytes && !out_host)) return TSX_HIP_ERANGE;
    HIP_TRY(hipSetDevice(device));
    BgzfDev dv;
    DevBuf<uint8_t> d_out;
    for (BgzfBatches b(ix, bgzf_batch_bytes()); !b.done(); b.next()) {
        const size_t nb = b.text();
        TSX_TRY(grow((hipStream_t) nullptr, d_out, nb + 256));
        TSX_TRY(inflate_batch((const uint8_t *)gz, n, ix, b.m0, b.m1, dv, d_out.get(), nullptr));
        if (nb && hipMemcpy((uint8_t *)out_host + ix.out_off[b.m0], d_out.get(), nb, hipMemcpyDeviceToHost) != hipSuccess) {
            g_last_error = "hipMemcpy of the inflated text failed";
            return TSX_HIP_EHIP;
        }
    }
    return TSX_HIP_OK;
}

// ---- pieces cut at record boundaries, and the base rule's low-quality bitmap over them (tsx_baserule.h) -------------------
// min_qual_char reads the 4th line of a FASTQ record: FASTA tables refuse it.
static int base_rule_ok(const tsx_hip_map *m) {
    if (m->minq && m->p.line_mask != 3) {
        g_last_error = "min_qual_char needs FASTQ records (4 lines): a FASTA text has no quality line";
        return TSX_HIP_EINVAL;
    }
    return TSX_HIP_OK;
}

// A non-empty line and its '\n' are two bytes: no text of n bytes holds more records than this.
static uint64_t max_records(const tsx_hip_map *m, uint64_t n) { return n / (2 * ((uint64_t)m->p.line_mask + 1)) + 2; }
// What turns a line index into a record index: 4 lines a record (FASTQ) or 2.
static uint32_t line_shift(const tsx_hip_map *m) { return m->p.line_mask == 3 ? 2u : 1u; }

// m->d_qmap.get() = the low-quality bitmap of d_text[0, n), a text that starts at a record boundary.  Uses the map's line
// scratch (d_tile, word 0 of d_carry) and waits once, for the line count.  The scan launches get it as qmap_cur.
static int build_qmap(tsx_hip_map *m, const uint8_t *d_text, uint64_t n, hipStream_t st) {
    if (n >= ((uint64_t)1 << 33)) { g_last_error = "min_qual_char: a text of 8 GiB or more"; return TSX_HIP_ERANGE; }
    const size_t words = (size_t)(n + 15) / 16 + 16;
    int rc = grow(st, m->d_qmap, words * 2);
    if (rc != TSX_HIP_OK) return rc;
    HIP_TRY(hipMemsetAsync(m->d_qmap.get(), 0, words * 2, st));
    if (n == 0) return TSX_HIP_OK;
    HIP_TRY(hipMemsetAsync(m->d_carry.get(), 0, sizeof(uint32_t), st));
    if ((rc = line_pass(m, d_text, n, n, 0, st)) != TSX_HIP_OK) return rc;
    uint32_t lines = 0;
    HIP_TRY(hipMemcpyAsync(&lines, m->d_carry.get(), sizeof lines, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const uint64_t nrec = (uint64_t)lines / 4 + 1, ntiles = (n + TILE - 1) / TILE;
    if ((rc = grow(st, m->d_qrec, (size_t)nrec * QR_N * 8)) != TSX_HIP_OK) return rc;
    HIP_TRY(hipMemsetAsync(m->d_qrec.get(), 0, (size_t)nrec * QR_N * 8, st));
    hipLaunchKernelGGL(qual_lines_kernel, dim3((uint32_t)std::min<uint64_t>(ntiles, (uint64_t)m->cus * 8)), dim3(NT), 0, st,
                       d_text, n, (const uint32_t *)m->d_tile.get(), ntiles, (const uint32_t *)m->d_carry.get(), m->d_qrec.get(), nrec);
    hipLaunchKernelGGL(qual_bits_kernel, dim3(grid_for(m, nrec * 16, 8)), dim3(NT), 0, st, d_text,
                       (const unsigned long long *)m->d_qrec.get(), nrec, m->minq, m->d_qmap.get());
    HIP_TRY(hipGetLastError());
    return TSX_HIP_OK;
}

// qmap_cur is set only for the launches of one call: the rule may change between calls.
struct QmapScope {
    tsx_hip_map *m;
    explicit QmapScope(tsx_hip_map *mm) : m(mm) {}
    ~QmapScope() { m->qmap_cur = nullptr; }
};

// Scratch common to the calls that work on a text piece by piece: the piece on the device, its record spans (for the
// calls that cut by them), the words the scans and the filters report in, their pinned copy.  The scratch of a call
// (QueryBufs, TrimBufs, MedianBufs) embeds it BEHIND its own buffers: the destructor here waits for the stream before
// any of them is released.
struct PieceBufs {
    DevBuf<uint8_t> text;
    DevBuf<unsigned long long> rspan;              // record spans
    DevBuf<unsigned long long> info;               // cut, records, open, total, line base (0), kept; the trim: bases in, bases kept
    PinBuf<unsigned long long> h_info;
    Event ev;                                      // info[3..] has been copied back
    hipStream_t st;
    explicit PieceBufs(hipStream_t s) : st(s) {}
    ~PieceBufs() { (void)hipStreamSynchronize(st); }   // nothing queued may outlive the buffers
    int init() {
        TSX_TRY(info.alloc(8 * sizeof(unsigned long long)));
        HIP_TRY(hipMemsetAsync(info.get(), 0, 8 * sizeof(unsigned long long), st));
        TSX_TRY(h_info.alloc(8 * sizeof(unsigned long long)));
        return ev.create();
    }
};

// The scan half of a piece [0, len) of text in device memory that starts at a record boundary: the line pass and the
// record scan into info[0..2] (cut, records, open), with the record spans when `span` is given.  Queued, not waited for.
static int piece_scan(tsx_hip_map *m, const uint8_t *d_text, uint64_t len, bool last, unsigned long long *info,
                      DevBuf<unsigned long long> *span, hipStream_t st) {
    const uint32_t lpr = m->p.line_mask + 1;
    const uint64_t ntiles = (len + TILE - 1) / TILE, span_cap = max_records(m, len);
    int rc;
    HIP_TRY(hipMemsetAsync(m->d_carry.get(), 0, sizeof(uint32_t), st));
    if ((rc = line_pass(m, d_text, len, len, 0, st)) != TSX_HIP_OK) return rc;
    if (span && (rc = grow(st, *span, span_cap * 16)) != TSX_HIP_OK) return rc;
    hipLaunchKernelGGL(record_scan_kernel, dim3((uint32_t)std::min<uint64_t>(ntiles, (uint64_t)m->cus * 8)), dim3(NT), 0, st,
                       d_text, len, (const uint32_t *)m->d_tile.get(), ntiles, (const uint32_t *)m->d_carry.get(), lpr, last ? 1 : 0,
                       info, span ? span->get() : (unsigned long long *)nullptr, span ? span_cap : (uint64_t)0);
    HIP_TRY(hipGetLastError());
    return TSX_HIP_OK;
}

// The front end of every piece [0, len) of text in device memory that starts at a record boundary: piece_scan (the
// spans in p.rspan when `spans`), then the ONE wait of a piece, for where its last whole record ends, its records and
// whether the last one lacks its '\n'.  An empty piece: nothing.
static int piece_front(tsx_hip_map *m, PieceBufs &p, const uint8_t *d_text, uint64_t len, bool last, bool spans, uint64_t &cut,
                       uint64_t &nrec, bool &open) {
    cut = nrec = 0; open = false;
    if (len == 0) return TSX_HIP_OK;
    TSX_TRY(piece_scan(m, d_text, len, last, p.info.get(), spans ? &p.rspan : nullptr, p.st));
    const unsigned long long *h_info = p.h_info.get();
    HIP_TRY(hipMemcpyAsync(p.h_info.get(), p.info.get(), 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, p.st));
    HIP_TRY(hipStreamSynchronize(p.st));
    cut = h_info[0]; nrec = h_info[1]; open = h_info[2] != 0;
    return TSX_HIP_OK;
}

// A quality rule: the bitmap of the whole records d_text[0, cut) for the launches that follow (its line pass over
// [0, cut) rewrites d_tile with the same values).  The caller holds a QmapScope.
static int piece_qmap(tsx_hip_map *m, const uint8_t *d_text, uint64_t cut, hipStream_t st) {
    if (!m->minq) return TSX_HIP_OK;
    TSX_TRY(build_qmap(m, d_text, cut, st));
    m->qmap_cur = m->d_qmap.get();
    return TSX_HIP_OK;
}

// The text of a BGZF file in pieces cut at record boundaries, batch by batch on `st`.  The unfinished last record of a
// batch is carried into the next one instead of a k-1 byte halo: the batch is inflated behind it, behind newlines that
// align the piece to 16 bytes (empty lines are no lines), and 256 newlines follow the text.  Then
//   work(piece, len, last, cut)      queues the call's work on the whole records piece[0, cut) and waits once, for the cut
// (the whole piece when last; 0 when the piece holds no whole record: it is carried whole).  What lies behind the cut is
// the next carry; more than carry_max bytes of it (only a quality-rule count sets a limit): ERANGE.  On an inflate error
// the work of the batches before it stands.  Nothing queued outlives the buffers: every way out waits for the stream.
template <class Work>
static int bgzf_record_pieces(const uint8_t *gz, size_t n, const BgzfIndex &ix, size_t carry_max, hipStream_t st, Work work) {
    BgzfDev dv;
    DevBuf<uint8_t> txt, tail;
    SyncAtExit wait(st);
    size_t r = 0;   // bytes of the carried record in `tail`
    for (BgzfBatches b(ix, bgzf_batch_bytes()); !b.done(); b.next()) {
        const size_t ra = (r + 15) & ~(size_t)15, len = ra + b.text();
        TSX_TRY(grow(st, txt, len + 256));
        uint8_t *const piece = txt.get();
        TSX_TRY(inflate_batch(gz, n, ix, b.m0, b.m1, dv, piece + ra, st));
        if (ra > r) HIP_TRY(hipMemsetAsync(piece, '\n', ra - r, st));
        if (r) HIP_TRY(hipMemcpyAsync(piece + ra - r, tail.get(), r, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemsetAsync(piece + len, '\n', 256, st));
        uint64_t cut = 0;
        TSX_TRY(work(piece, (uint64_t)len, b.last(), cut));
        r = b.last() ? 0 : len - (size_t)cut;
        if (r > carry_max) {
            g_last_error = "min_qual_char: a record longer than " + std::to_string(carry_max) + " bytes in a BGZF file";
            return TSX_HIP_ERANGE;
        }
        if (r) {
            TSX_TRY(grow(st, tail, r));
            HIP_TRY(hipMemcpyAsync(tail.get(), piece + cut, r, hipMemcpyDeviceToDevice, st));
        }
        HIP_TRY(hipStreamSynchronize(st));   // (txt is refilled next)
    }
    return TSX_HIP_OK;
}

// ==== counting: a text into the table ======================================================================================

// ---- tables above 2^32 slots (l - S > 18): built slab by slab ----------------------------------------------------------
// 1. every window of the text is DESCRIBED once (line pass + strip_desc_kernel, long descriptions: 32 bytes per 64 start
//    positions), the descriptions of all windows stay in HBM;
// 2. for every slab: the owner-filtered walk over every window's descriptions keeps the slab's keys and partitions them by
//    radix level 1 (one set of sub-lists per window), then ONE level 2 + build for the slab -- a slab is to this loop what a
//    shard is to a GPU of a multi-GPU run, and the per-slab view of the table parameters is a shard's view (l = slab bits,
//    shard = slab number) with the table pointers moved to the slab and pos_base = its first slot.
// The text is walked slab_count times (rolling work only, ~2 ms per 1e9 positions); every key makes its two trips once.
static const size_t DEV_WINDOW_DEFAULT = (size_t)4 << 30;
static size_t dev_window_bytes() {
    size_t w = DEV_WINDOW_DEFAULT;
    if (const char *e = getenv("TSX_HIP_DEV_WINDOW")) {  // tests exercise the window seams
        const long long v = atoll(e);
        if (v >= 4096) w = ((size_t)v + 15) & ~(size_t)15;
    }
    return w;
}

// ---- a quality rule on a host text: counted piece by piece, cut at record boundaries ------------------------------------
// One piece d[0, len) of a text cut at record boundaries (a quality rule): where its last whole record ends (cut; the
// whole piece when last; 0 when it holds no whole record), then the bitmap and the count of [0, cut).  Waits for the cut.
static int count_record_piece(tsx_hip_map *m, const uint8_t *d, uint64_t len, bool last, hipStream_t st, uint64_t &cut) {
    cut = last ? len : 0;
    if (len == 0) return TSX_HIP_OK;
    if (!last) {
        TSX_TRY(grow(st, m->d_qrec, 64));
        unsigned long long *info = m->d_qrec.get();   // (read back before build_qmap reuses it)
        TSX_TRY(piece_scan(m, d, len, false, info, nullptr, st));
        unsigned long long h[2] = {0, 0};
        HIP_TRY(hipMemcpyAsync(h, info, sizeof h, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        cut = h[1] ? h[0] : 0;
        if (cut == 0) return TSX_HIP_OK;
    }
    QmapScope qs(m);
    TSX_TRY(piece_qmap(m, d, cut, st));
    HIP_TRY(hipMemsetAsync(m->d_carry.get(), 0, sizeof(uint32_t), st));
    return run_fastq_piece(m, d, cut, cut, 0, st);
}

// tsx_hip_count_fastq_host under a quality rule: pieces of m->piece bytes cut at record boundaries, one at a time (where
// a piece starts depends on the cut of the one before: nothing to overlap); the next piece starts where the last whole
// record of this one ends.  A record longer than a piece: ERANGE.
static int count_host_records(tsx_hip_map *m, const char *text, size_t n) {
    TSX_TRY(ensure_staging(m, n));
    hipStream_t st = m->stream.get();
    for (size_t off = 0; off < n;) {
        const size_t len = std::min(m->piece, n - off);
        const bool last = off + len == n;
        TSX_TRY(stage_upload(m, 0, text + off, len, st));
        uint64_t cut = 0;
        TSX_TRY(count_record_piece(m, m->d_stage[0].get(), len, last, st, cut));
        if (cut == 0) {
            g_last_error = "min_qual_char: a record longer than a host piece (" + std::to_string(m->piece) + " bytes)";
            return TSX_HIP_ERANGE;
        }
        HIP_TRY(hipStreamSynchronize(st));   // (the staging buffers are reused by the next piece)
        off += cut;
    }
    return tsx_hip_sync(m);
}

// ---- FASTQ: the slab-by-slab build (above), device texts in windows, BGZF batches, host pieces ----------------------------
static int count_slabs(tsx_hip_map *m, const uint8_t *base, size_t n, hipStream_t st, const uint16_t *qmap) {
    const int sb = slab_bits(m);
    const uint32_t nslab = 1u << sb;
    const size_t halo = (size_t)m->p.k - 1, WIN = dev_window_bytes();
    const uint32_t nwin = (uint32_t)std::max<size_t>(1, (n + WIN - 1) / WIN);
    // descriptions of all windows, back to back (window w at word offset doff[w] of 32-byte descriptions)
    std::vector<size_t> doff(nwin + 1, 0);
    for (uint32_t w = 0; w < nwin; ++w) doff[w + 1] = doff[w] + std::min(WIN, n - (size_t)w * WIN) / 64 + 4096;
    // (scratch of the map, grown on demand: allocating and freeing gigabytes per call costs more than the kernels)
    int rc = grow(st, m->d_slabdesc, doff[nwin] * 32 + (size_t)(nwin + 1) * 8);
    if (rc != TSX_HIP_OK) return rc;
    uint4 *d_desc = reinterpret_cast<uint4 *>(m->d_slabdesc.get());
    unsigned long long *d_cnt = reinterpret_cast<unsigned long long *>(m->d_slabdesc.get() + doff[nwin] * 32);
    auto done = [&](int code) { m->ev_open.clear(); return code; };
    if (hipMemsetAsync(d_cnt, 0, (size_t)(nwin + 1) * 8, st) != hipSuccess) return done(TSX_HIP_EHIP);
    for (uint32_t w = 0; w < nwin && rc == TSX_HIP_OK; ++w) {
        const size_t off = (size_t)w * WIN, own = std::min(WIN, n - off), len = std::min(own + halo, n - off);
        DescOut dsc;
        dsc.out = d_desc + doff[w] * 2; dsc.cap = doff[w + 1] - doff[w]; dsc.count = d_cnt + w; dsc.sum = d_cnt + nwin; dsc.long_desc = 1;
        m->qmap_cur = qmap ? qmap + off / 16 : nullptr;   // (windows start at multiples of 16)
        rc = run_fastq_piece(m, base + off, len, own, off > 0 ? -1 : 0, st, ShardOut(), HotOut(), dsc);
    }
    m->qmap_cur = nullptr;
    if (rc != TSX_HIP_OK) return done(rc);
    std::vector<unsigned long long> cnt(nwin + 1);
    if (hipMemcpyAsync(cnt.data(), d_cnt, (size_t)(nwin + 1) * 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) return done(TSX_HIP_EHIP);
    m->ev_open.clear();   // (the description calls queued timing tuples for a sharded build that never comes)
    const uint64_t kmers = cnt[nwin];
    if (kmers == 0) return done(TSX_HIP_OK);
    const TableParams whole = m->p;
    const bool fresh = m->fresh;
    const size_t est = (size_t)(kmers / nslab + kmers / nslab / 8) + 65536;
    for (uint32_t s = 0; s < nslab && rc == TSX_HIP_OK; ++s) {
        TableParams &v = m->p;     // the slab's view
        v = whole;
        v.l = whole.l - sb;
        v.slot_mask = (1ULL << v.l) - 1ULL;
        v.shard = s;
        v.pos_base = (uint64_t)s << v.l;
        v.table = whole.table + ((uint64_t)s << v.l);
        v.seg_dirty = whole.seg_dirty + ((uint64_t)s << (v.l - v.S));
        m->fresh = fresh;
        Event *ev = nullptr;   // the slab's own tuple: no line pass, no scan -- its walks count as level 1
        if ((rc = timing_open(m, ev, st)) != TSX_HIP_OK) break;
        if (ev) rc = timing_record(ev, EV_SCAN, EV_PART, st);
        for (uint32_t w = 0; w < nwin && rc == TSX_HIP_OK; ++w)
            rc = shard_walk(m, d_desc + doff[w] * 2, (size_t)cnt[w], 1, w, nwin, est, nullptr, st);
        if (rc == TSX_HIP_OK) {
            if (!m->sh_pl || !m->sh_pl->fused) rc = TSX_HIP_EINVAL;
            else rc = run_partition_build(m, *m->sh_pl, nullptr, nullptr, 0, st, ev);
        }
        if (rc == TSX_HIP_OK) rc = timing_close(ev, EV_END, st);
    }
    m->p = whole;
    if (rc == TSX_HIP_OK) m->fresh = false;
    return done(rc);
}

// A table built slab by slab walks the whole text once per slab: the host forms send the text to the device in one piece
// (newlines behind it) and call their device form.
template <class DeviceForm>
static int count_resident(tsx_hip_map *m, const char *text, size_t n, DeviceForm device_form) {
    DevBuf<uint8_t> d_text;
    TSX_TRY(d_text.alloc(n + 256));
    SyncAtExit wait(m->stream.get());   // nothing queued may outlive the text
    if (hipMemcpy(d_text.get(), text, n, hipMemcpyHostToDevice) != hipSuccess || hipMemset(d_text.get() + n, '\n', 256) != hipSuccess) return TSX_HIP_EHIP;
    TSX_TRY(device_form(m, d_text.get(), n, nullptr));
    return tsx_hip_sync(m);
}

// Device texts are processed in windows so that the partition scratch (about
// 10 bytes per text byte) stays bounded; windows overlap by the k-1 byte halo
// exactly like the host pieces.
// An armed prefilter (tsx_prefilter.h) is consulted by the atomic path of a whole table alone.  Checked before anything
// is queued.
// Pass 1 writes the filters on whatever stream it was given, pass 2 reads B on whatever stream it is given.  Before
// pick_stream of an armed count: the map's stream goes behind the last caller's stream (join_foreign), and a caller's
// `stream` behind the map's -- so B is complete before it is read, whichever streams the two passes ran on.
static int prefilter_order(tsx_hip_map *m, void *stream) {
    join_foreign(m, false);
    if (stream && (hipStream_t)stream != m->stream.get()) {
        HIP_TRY(hipEventRecord(m->pf_ev.get(), m->stream.get()));
        HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, m->pf_ev.get(), 0));
    }
    return TSX_HIP_OK;
}

static int prefilter_count_ok(const tsx_hip_map *m) {
    if (!m->pf_armed) return TSX_HIP_OK;
    if (m->p.lg != m->p.l) { g_last_error = "prefilter armed: a map created with shard_bits > 0"; return TSX_HIP_EINVAL; }
    if (slab_bits(m)) { g_last_error = "prefilter armed: a table above 2^32 slots is built slab by slab, without the filter"; return TSX_HIP_EINVAL; }
    return TSX_HIP_OK;
}

extern "C" int tsx_hip_count_fastq_device(tsx_hip_map *m, const void *dev_text, size_t n, void *stream) {
    if (!m || (!dev_text && n) || ((uintptr_t)dev_text & 15)) return TSX_HIP_EINVAL;
    TSX_TRY(prefilter_count_ok(m));
    if (m->p.lg != m->p.l) return TSX_HIP_EINVAL;   // a shard: keys of other owners must travel (shard_scan / shard_build)
    if (n) m->used = true;
    HIP_TRY(hipSetDevice(m->device));
    if (m->pf_armed) TSX_TRY(prefilter_order(m, stream));   // behind pass 1, on whichever stream it ran
    hipStream_t st = pick_stream(m, stream);
    const uint8_t *base = (const uint8_t *)dev_text;
    // a quality rule: the bitmap of the whole (resident) text, read by each window at its offset
    int rcq = base_rule_ok(m);
    if (rcq == TSX_HIP_OK && m->minq) rcq = build_qmap(m, base, n, st);
    if (rcq != TSX_HIP_OK) return rcq;
    const uint16_t *qmap = m->minq ? m->d_qmap.get() : nullptr;
    QmapScope qs(m);
    HIP_TRY(hipMemsetAsync(m->d_carry.get(), 0, 64, st));
    const size_t halo = (size_t)m->p.k - 1;
    const size_t DEV_WINDOW = dev_window_bytes();
    if (slab_build_wanted(m, n)) return count_slabs(m, base, n, st, qmap);
    for (size_t off = 0; off < n || off == 0; off += DEV_WINDOW) {
        const size_t own = std::min(DEV_WINDOW, n - off);
        const size_t len = std::min(own + halo, n - off);
        m->qmap_cur = qmap ? qmap + off / 16 : nullptr;   // (windows start at multiples of 16)
        // whether the previous window ends inside a line is read on the device (the byte in front of this one)
        int rc = run_fastq_piece(m, base + off, len, own, off > 0 ? -1 : 0, st);
        if (rc != TSX_HIP_OK) return rc;
        if (n == 0) break;
    }
    return TSX_HIP_OK;
}

// The text never exists as a whole: batch b is inflated into one of two buffers BEHIND the last BGZF_PRE + 16 bytes
// of batch b-1, and counted as a piece that owns the start positions up to BGZF_PRE bytes before its end (the last
// batch: all of them) -- the k-1 bytes a window needs behind its start are always there, the byte in front of a
// piece (is its first line open?) as well.  On an inflate error the table holds the batches before it.
static const size_t BGZF_PRE = 256;   // >= k - 1, a multiple of 16

// tsx_hip_count_fastq_bgzf_host under a quality rule: batch by batch on the map's stream.  The unfinished last record of
// a batch is carried into the next one instead of a k-1 byte halo: it goes in front of the next batch's text, behind
// newlines that align the piece to 16 bytes (empty lines are dropped).  A record longer than BGZF_CARRY: ERANGE.
static const size_t BGZF_CARRY = (size_t)8 << 20;

static int count_bgzf_records(tsx_hip_map *m, const uint8_t *gz, size_t n, const BgzfIndex &ix, hipStream_t st) {
    return bgzf_record_pieces(gz, n, ix, BGZF_CARRY, st, [&](const uint8_t *piece, uint64_t len, bool last, uint64_t &cut) {
        return count_record_piece(m, piece, len, last, st, cut);
    });
}

extern "C" int tsx_hip_count_fastq_bgzf_host(tsx_hip_map *m, const void *gz, size_t n) {
    if (!m || (!gz && n)) return TSX_HIP_EINVAL;
    TSX_TRY(prefilter_count_ok(m));
    if (m->p.lg != m->p.l) return TSX_HIP_EINVAL;   // see tsx_hip_count_fastq_device
    if (n) m->used = true;
    BgzfIndex ix;
    if (!bgzf_index((const uint8_t *)gz, n, ix)) { g_last_error = "not a BGZF file (no BC extra field in every gzip member)"; return TSX_HIP_EINVAL; }
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t st = m->stream.get();
    join_foreign(m, false);
    if (int rcq = base_rule_ok(m)) return rcq;
    if (m->minq) return count_bgzf_records(m, (const uint8_t *)gz, n, ix, st);
    HIP_TRY(hipMemsetAsync(m->d_carry.get(), 0, 64, st));
    const size_t head = BGZF_PRE + 16;
    BgzfBatches bt(ix, bgzf_batch_bytes());
    // (the inflate stream is declared first: it outlives the buffers it fills)
    Stream inflate_stream;
    Event counted[2];
    BgzfDev dv;
    DevBuf<uint8_t> txt[2];
    const size_t buf_bytes = head + bt.biggest() + 256;
    int rc = TSX_HIP_OK;
    for (int i = 0; i < 2 && rc == TSX_HIP_OK; ++i)   // (the second buffer only when a second batch exists)
        if ((i == 0 || !bt.last()) && txt[i].alloc(buf_bytes) != TSX_HIP_OK) {
            g_last_error = "hipMalloc of a BGZF text buffer failed";
            rc = TSX_HIP_ENOMEM;
        }
    uint8_t *const d_txt[2] = {txt[0].get(), txt[1].get()};
    // Batch i + 1 is copied to the device and inflated on a stream of its own while batch i is counted on the map's: the
    // inflate stream only waits for the count that last read the buffer it is about to fill (two batches back).
    if (rc == TSX_HIP_OK && d_txt[1] &&
        (inflate_stream.create() != TSX_HIP_OK || counted[0].create() != TSX_HIP_OK || counted[1].create() != TSX_HIP_OK)) {
        g_last_error = "hipStreamCreate for the BGZF inflate stream failed";
        rc = TSX_HIP_EHIP;
    }
    const hipStream_t st_inf = inflate_stream.get();
    size_t prev_len = 0;   // bytes of text in the previous batch's buffer, behind its head
    int b = 0;
    size_t nbatch = 0;
    for (; !bt.done() && rc == TSX_HIP_OK; bt.next(), b ^= 1, ++nbatch) {
        const size_t nb = bt.text();
        const bool first = bt.first(), last = bt.last();
        uint8_t *buf = d_txt[b];
        hipStream_t sti = st_inf ? st_inf : st;   // (one batch in all: everything on the map's stream)
        if (st_inf && nbatch >= 2 && hipStreamWaitEvent(st_inf, counted[b].get(), 0) != hipSuccess) { rc = TSX_HIP_EHIP; break; }
        rc = inflate_batch((const uint8_t *)gz, n, ix, bt.m0, bt.m1, dv, buf + head, sti);   // (returns when the text is there)
        if (rc != TSX_HIP_OK) break;
        if (!first) {   // the end of the text so far (it may reach back into the previous buffer's own head)
            if (hipMemcpyAsync(buf, d_txt[b ^ 1] + prev_len, head, hipMemcpyDeviceToDevice, st) != hipSuccess) { rc = TSX_HIP_EHIP; break; }
            // (the other buffer is free for the next batch's text only behind this copy as well)
            if (st_inf && hipEventRecord(counted[b ^ 1].get(), st) != hipSuccess) { rc = TSX_HIP_EHIP; break; }
        }
        if (hipMemsetAsync(buf + head + nb, '\n', 256, st) != hipSuccess) { rc = TSX_HIP_EHIP; break; }
        // piece: from `from` (16-byte aligned) to the end of this batch's text; it owns all start positions but the
        // last BGZF_PRE (they belong to the next piece, which sees them again behind its own head)
        const size_t from = first ? head : 16, len = head + nb - from;
        const size_t own = last ? len : (len > BGZF_PRE ? len - BGZF_PRE : 0);
        rc = run_fastq_piece(m, buf + from, len, own, first ? 0 : -1, st);
        if (rc == TSX_HIP_OK && st_inf && hipEventRecord(counted[b].get(), st) != hipSuccess) rc = TSX_HIP_EHIP;
        prev_len = nb;
    }
    hipError_t e = hipStreamSynchronize(st);   // nothing queued may outlive the buffers
    if (st_inf) (void)hipStreamSynchronize(st_inf);
    if (rc == TSX_HIP_OK && e != hipSuccess) { g_last_error = hipGetErrorString(e); rc = TSX_HIP_EHIP; }
    return rc;
}

extern "C" int tsx_hip_count_fastq_host(tsx_hip_map *m, const char *text, size_t n) {
    if (!m || (!text && n)) return TSX_HIP_EINVAL;
    TSX_TRY(prefilter_count_ok(m));
    if (m->p.lg != m->p.l) return TSX_HIP_EINVAL;   // see tsx_hip_count_fastq_device
    if (n) m->used = true;
    HIP_TRY(hipSetDevice(m->device));
    if (m->pf_armed) join_foreign(m, false);   // behind a pass 1 on a caller's stream
    HIP_TRY(hipStreamSynchronize(m->stream.get()));
    if (slab_build_wanted(m, n)) return count_resident(m, text, n, tsx_hip_count_fastq_device);
    int rc = base_rule_ok(m);
    if (rc != TSX_HIP_OK) return rc;
    if (m->minq) return count_host_records(m, text, n);
    hipStream_t st = m->stream.get();
    HIP_TRY(hipMemsetAsync(m->d_carry.get(), 0, 64, st));
    // Pieces own m->piece start positions and carry a k-1 byte halo so that
    // windows beginning near the end of a piece see their last bytes.
    return staged_pieces(m, text, n, m->piece, (size_t)m->p.k - 1, [&](const uint8_t *d_piece, size_t len, size_t own, int head_open) {
        return run_fastq_piece(m, d_piece, len, own, head_open, st);
    });
}

// ---- wrapped FASTA: sequence lines joined on the device (tsx_fasta.h), then counted as two-line text ----------------
static const size_t FA_PIECE_MAX = (size_t)1 << 31;   // output positions of a piece are 32 bits wide
static const size_t FA_TAIL = 256;                    // newlines behind a piece's bound
// Bytes the two-line text of a piece of n bytes can take: the text (+ 2), ">\n" + k - 1 carried bases; a multiple of 16.
static inline size_t fa_bound(size_t n, int k) { return (n + (size_t)k + 16 + 15) & ~(size_t)15; }

// Unwraps d_text[0, n) (16-byte aligned, 0 < n <= FA_PIECE_MAX) behind the carry in d_carry (FA_CARRY_BYTES, then
// FA_INFO_WORDS info words) into d_out[0, out_end): the two-line text, then '\n' up to out_end.  Leaves the carry of the
// next piece and the output's size (info word 0) on the device; does not wait.
static int fasta_unwrap(const uint8_t *d_text, uint64_t n, uint32_t *d_carry, uint32_t kminus1, DevBuf<uint32_t> &ws,
                        uint8_t *d_out, uint64_t out_end, int cus, hipStream_t st) {
    const uint64_t ntiles = (n + TILE - 1) / TILE, nchunks = (ntiles + SCAN_CHUNK - 1) / SCAN_CHUNK;
    TSX_TRY(grow(st, ws, (size_t)ntiles * 24 + (size_t)nchunks * (FA_CHUNK_WORDS + 2) * 4 + 64));
    uint32_t *const d_ws = ws.get();
    uint4 *summ = reinterpret_cast<uint4 *>(d_ws);
    uint32_t *tile_state = d_ws + ntiles * 4, *tile_pos = tile_state + ntiles, *chunk_fn = tile_pos + ntiles;
    uint32_t *chunk_in = chunk_fn + nchunks * FA_CHUNK_WORDS, *info = d_carry + FA_CARRY_BYTES / 4;
    const uint32_t cap = (uint32_t)std::min<uint64_t>(out_end, 0xFFFFFFF0u);
    const int g = (int)std::min<uint64_t>(ntiles, (uint64_t)cus * 8);
    hipLaunchKernelGGL(fasta_summary_kernel, dim3(g), dim3(NT), 0, st, d_text, n, (const uint32_t *)d_carry, summ, ntiles);
    hipLaunchKernelGGL(fasta_chunk_kernel, dim3((uint32_t)nchunks), dim3(SCAN_CHUNK), 0, st, (const uint4 *)summ, ntiles, chunk_fn);
    hipLaunchKernelGGL(fasta_chunk_scan_kernel, dim3(1), dim3(NT), 0, st, (const uint32_t *)chunk_fn, (uint32_t)nchunks,
                       (const uint32_t *)d_carry, kminus1, chunk_in, info, d_out, cap);
    hipLaunchKernelGGL(fasta_tile_scan_kernel, dim3((uint32_t)nchunks), dim3(SCAN_CHUNK), 0, st, (const uint4 *)summ, ntiles,
                       (const uint32_t *)chunk_in, tile_state, tile_pos);
    hipLaunchKernelGGL(fasta_emit_kernel, dim3(g), dim3(NT), 0, st, d_text, n, (const uint32_t *)d_carry, (const uint32_t *)tile_state,
                       (const uint32_t *)tile_pos, ntiles, d_out, cap);
    hipLaunchKernelGGL(fasta_finish_kernel, dim3(1), dim3(128), 0, st, d_text, n, (const uint32_t *)info, (const uint8_t *)d_out, kminus1,
                       d_carry);
    hipLaunchKernelGGL(fasta_fill_kernel, dim3((uint32_t)std::min<uint64_t>(out_end / (16 * NT) + 1, (uint64_t)cus * 8)), dim3(NT), 0, st,
                       (const uint32_t *)info, d_out, out_end);
    HIP_TRY(hipGetLastError());
    return TSX_HIP_OK;
}

// The wrapped-FASTA entry points count two-line records whatever tsx_hip_set_record_lines says, and put it back.
struct FastaScope {
    tsx_hip_map *m;
    uint32_t mask;
    explicit FastaScope(tsx_hip_map *mm) : m(mm), mask(mm->p.line_mask) { m->p.line_mask = 1u; }
    ~FastaScope() { m->p.line_mask = mask; }
};

static int fasta_args_ok(const tsx_hip_map *m) {
    if (m->p.lg != m->p.l) { g_last_error = "wrapped FASTA: a map created with shard_bits > 0"; return TSX_HIP_EINVAL; }
    if (m->minq) { g_last_error = "wrapped FASTA: min_qual_char needs FASTQ records (a FASTA text has no quality line)"; return TSX_HIP_EINVAL; }
    if (m->pf_armed) { g_last_error = "wrapped FASTA: a prefilter is armed (pass 1 reads FASTQ or two-line records)"; return TSX_HIP_EINVAL; }
    return TSX_HIP_OK;
}
static int fasta_begin(tsx_hip_map *m, hipStream_t st) {   // the carry of a new text: at a line start, no open record
    if (!m->d_fa_carry.get()) TSX_TRY(m->d_fa_carry.alloc(FA_CARRY_BYTES + FA_INFO_WORDS * 4));
    HIP_TRY(hipMemsetAsync(m->d_fa_carry.get(), 0, FA_CARRY_BYTES + FA_INFO_WORDS * 4, st));
    return TSX_HIP_OK;
}

// One piece of a wrapped text, behind the carry: unwrapped into the map's scratch and counted at its upper-bound length
// (what the unwrap did not write there is newlines: empty lines), so that nothing is read back.
static int fasta_count_piece(tsx_hip_map *m, const uint8_t *d_text, uint64_t n, hipStream_t st) {
    if (n == 0) return TSX_HIP_OK;
    const size_t ub = fa_bound(n, m->p.k);
    int rc = grow(st, m->d_fa_out, ub + FA_TAIL);
    if (rc == TSX_HIP_OK)
        rc = fasta_unwrap(d_text, n, m->d_fa_carry.get(), (uint32_t)m->p.k - 1u, m->d_fa_ws, m->d_fa_out.get(), ub + FA_TAIL, m->cus, st);
    if (rc != TSX_HIP_OK) return rc;
    HIP_TRY(hipMemsetAsync(m->d_carry.get(), 0, 64, st));   // (every unwrapped piece starts at a record boundary)
    return run_fastq_piece(m, m->d_fa_out.get(), ub, ub, 0, st);
}

extern "C" int tsx_hip_count_fasta_device(tsx_hip_map *m, const void *dev_text, size_t n, void *stream) {
    if (!m || (!dev_text && n) || ((uintptr_t)dev_text & 15)) return TSX_HIP_EINVAL;
    if (int rca = fasta_args_ok(m)) return rca;
    if (n) m->used = true;
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t st = pick_stream(m, stream);
    int rc = fasta_begin(m, st);
    if (rc != TSX_HIP_OK) return rc;
    FastaScope fs(m);
    const uint8_t *base = (const uint8_t *)dev_text;
    const size_t WIN = std::min(dev_window_bytes(), FA_PIECE_MAX);
    if (!slab_build_wanted(m, n)) {
        for (size_t off = 0; off < n && rc == TSX_HIP_OK; off += WIN) rc = fasta_count_piece(m, base + off, std::min(WIN, n - off), st);
        return rc;
    }
    // a table built slab by slab walks the whole text once per slab: every window's two-line text stays, back to back
    size_t total = 0;
    for (size_t off = 0; off < n; off += WIN) total += fa_bound(std::min(WIN, n - off), m->p.k);
    if ((rc = grow(st, m->d_fa_out, total + FA_TAIL)) != TSX_HIP_OK) return rc;
    size_t at = 0;
    for (size_t off = 0; off < n && rc == TSX_HIP_OK; off += WIN) {
        const size_t len = std::min(WIN, n - off), ub = fa_bound(len, m->p.k);
        rc = fasta_unwrap(base + off, len, m->d_fa_carry.get(), (uint32_t)m->p.k - 1u, m->d_fa_ws, m->d_fa_out.get() + at,
                          ub + (off + len == n ? FA_TAIL : 0), m->cus, st);
        at += ub;
    }
    if (rc != TSX_HIP_OK) return rc;
    return tsx_hip_count_fastq_device(m, m->d_fa_out.get(), total, stream);
}

extern "C" int tsx_hip_count_fasta_host(tsx_hip_map *m, const char *text, size_t n) {
    if (!m || (!text && n)) return TSX_HIP_EINVAL;
    if (int rca = fasta_args_ok(m)) return rca;
    if (n) m->used = true;
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipStreamSynchronize(m->stream.get()));
    if (slab_build_wanted(m, n)) return count_resident(m, text, n, tsx_hip_count_fasta_device);
    hipStream_t st = m->stream.get();
    TSX_TRY(fasta_begin(m, st));
    FastaScope fs(m);
    // pieces are cut anywhere and overlap nowhere: what a k-mer across the cut needs travels in the carry
    return staged_pieces(m, text, n, std::min(m->piece, FA_PIECE_MAX), 0, [&](const uint8_t *d_piece, size_t len, size_t, int) {
        return fasta_count_piece(m, d_piece, len, st);
    });
}

// Batch after batch on the map's stream: inflated, unwrapped behind the carry, counted.
extern "C" int tsx_hip_count_fasta_bgzf_host(tsx_hip_map *m, const void *gz, size_t n) {
    if (!m || (!gz && n)) return TSX_HIP_EINVAL;
    if (int rca = fasta_args_ok(m)) return rca;
    if (n) m->used = true;
    BgzfIndex ix;
    if (!bgzf_index((const uint8_t *)gz, n, ix)) { g_last_error = "not a BGZF file (no BC extra field in every gzip member)"; return TSX_HIP_EINVAL; }
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t st = m->stream.get();
    join_foreign(m, false);
    int rc = fasta_begin(m, st);
    if (rc != TSX_HIP_OK) return rc;
    FastaScope fs(m);
    BgzfBatches bt(ix, std::min(bgzf_batch_bytes(), FA_PIECE_MAX));
    BgzfDev dv;
    DevBuf<uint8_t> txt;
    if (txt.alloc(bt.biggest() + 256) != TSX_HIP_OK) { g_last_error = "hipMalloc of a BGZF text buffer failed"; return TSX_HIP_ENOMEM; }
    uint8_t *const d_txt = txt.get();
    for (; !bt.done() && rc == TSX_HIP_OK; bt.next()) {
        rc = inflate_batch((const uint8_t *)gz, n, ix, bt.m0, bt.m1, dv, d_txt, st);   // (behind the count of the batch before)
        if (rc == TSX_HIP_OK) rc = fasta_count_piece(m, d_txt, bt.text(), st);
    }
    hipError_t e = hipStreamSynchronize(st);   // nothing queued may outlive the buffers
    if (rc == TSX_HIP_OK && e != hipSuccess) { g_last_error = hipGetErrorString(e); rc = TSX_HIP_EHIP; }
    return rc == TSX_HIP_OK ? tsx_hip_sync(m) : rc;
}

extern "C" int tsx_hip_unwrap_fasta_host(int device, const char *text, size_t n, void *out_host, size_t out_cap, size_t *out_bytes) {
    if ((!text && n) || !out_bytes) return TSX_HIP_EINVAL;
    *out_bytes = n ? n + 2 : 0;   // (the bound, until the size is known)
    if (n >= ((size_t)1 << 32) - 64) { g_last_error = "unwrap_fasta: a text of 2^32 - 64 bytes or more"; return TSX_HIP_ERANGE; }
    if (n == 0) return TSX_HIP_OK;
    HIP_TRY(hipSetDevice(device));
    int cus = 256;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
    DevBuf<uint8_t> d_text, d_out;
    DevBuf<uint32_t> d_carry, d_ws;
    const size_t end = ((n + 2 + 15) & ~(size_t)15) + 16;
    TSX_TRY(d_text.alloc(n + 256));
    TSX_TRY(d_out.alloc(end));
    TSX_TRY(d_carry.alloc(FA_CARRY_BYTES + FA_INFO_WORDS * 4));
    HIP_TRY(hipMemcpy(d_text.get(), text, n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(d_carry.get(), 0, FA_CARRY_BYTES + FA_INFO_WORDS * 4));
    TSX_TRY(fasta_unwrap(d_text.get(), n, d_carry.get(), 0u, d_ws, d_out.get(), end, cus, nullptr));
    uint32_t total = 0;
    HIP_TRY(hipMemcpy(&total, d_carry.get() + FA_CARRY_BYTES / 4, 4, hipMemcpyDeviceToHost));
    *out_bytes = total ? (size_t)total + 1 : 0;   // the newline that ends the last record comes from the fill
    if (*out_bytes > out_cap || (*out_bytes && !out_host)) return TSX_HIP_ERANGE;
    if (*out_bytes) HIP_TRY(hipMemcpy(out_host, d_out.get(), *out_bytes, hipMemcpyDeviceToHost));
    return TSX_HIP_OK;
}

extern "C" int tsx_hip_add_kmers_device(tsx_hip_map *m, const void *dev_kmers, const void *dev_counts, size_t n,
                                        void *stream) {
    if (!m || (!dev_kmers && n)) return TSX_HIP_EINVAL;
    if (n == 0) return TSX_HIP_OK;
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t st = pick_stream(m, stream);
    int rcz = ensure_zeroed(m, st);
    if (rcz != TSX_HIP_OK) return rcz;
    const int grid = grid_for(m, n, 8);
    m->used = true;
    DISPATCH_CANON(m, DISPATCH_WK(m, hipLaunchKernelGGL((add_kmers_kernel<WKV, CANV>), dim3(grid), dim3(NT), 0, st, m->p,
                                                        (const uint64_t *)dev_kmers, (const uint64_t *)dev_counts, (uint64_t)n)));
    HIP_TRY(hipGetLastError());
    return TSX_HIP_OK;
}

extern "C" int tsx_hip_add_kmers_host(tsx_hip_map *m, const uint64_t *kmers, const uint64_t *counts, size_t n) {
    if (!m || (!kmers && n)) return TSX_HIP_EINVAL;
    if (n == 0) return TSX_HIP_OK;
    HIP_TRY(hipSetDevice(m->device));
    DevBuf<uint64_t> dk, dc;
    const size_t kb = n * (size_t)m->p.wk * 8;
    TSX_TRY(dk.alloc(kb));
    SyncAtExit wait(m->stream.get());   // nothing queued may outlive the buffers
    if (hipMemcpyAsync(dk.get(), kmers, kb, hipMemcpyHostToDevice, m->stream.get()) != hipSuccess) return TSX_HIP_EHIP;
    if (counts) {
        if (dc.alloc(n * 8) != TSX_HIP_OK) return TSX_HIP_ENOMEM;
        if (hipMemcpyAsync(dc.get(), counts, n * 8, hipMemcpyHostToDevice, m->stream.get()) != hipSuccess) return TSX_HIP_EHIP;
    }
    TSX_TRY(tsx_hip_add_kmers_device(m, dk.get(), dc.get(), n, nullptr));
    return tsx_hip_sync(m);
}

extern "C" int tsx_hip_get_counts_device(tsx_hip_map *m, const void *dev_kmers, size_t n, void *dev_counts_out,
                                         void *stream) {
    if (!m || ((!dev_kmers || !dev_counts_out) && n)) return TSX_HIP_EINVAL;
    if (n == 0) return TSX_HIP_OK;
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t st = pick_stream(m, stream);
    int rcz = ensure_zeroed(m, st);
    if (rcz != TSX_HIP_OK) return rcz;
    const int grid = grid_for(m, n, 8);
    DISPATCH_CANON(m, DISPATCH_WK(m, hipLaunchKernelGGL((get_counts_kernel<WKV, CANV>), dim3(grid), dim3(NT), 0, st, m->p,
                                                        (const uint64_t *)dev_kmers, (uint64_t)n, (uint64_t *)dev_counts_out,
                                                        (uint64_t *)nullptr)));
    HIP_TRY(hipGetLastError());
    return TSX_HIP_OK;
}

// Host-side lookups of a handful of k-mers (the reference calls getKmerCount one k-mer at a time,
// main.cpp:285-330) go through a small device scratch kept with the map instead of buffers of the call.
static const size_t SMALL_LOOKUP = 256;
static int lookup_host(tsx_hip_map *m, const uint64_t *kmers, size_t n, uint64_t *counts_out, uint64_t *slots_out) {
    if (!m || ((!kmers || !counts_out) && n)) return TSX_HIP_EINVAL;
    if (n == 0) return TSX_HIP_OK;
    HIP_TRY(hipSetDevice(m->device));
    join_foreign(m, false);
    int rcz = ensure_zeroed(m, m->stream.get());
    if (rcz != TSX_HIP_OK) return rcz;
    const size_t wk = (size_t)m->p.wk, kb = n * wk * 8;
    DevBuf<uint64_t> big_k, big_c;   // more than SMALL_LOOKUP k-mers: buffers of this call
    uint64_t *dk = nullptr, *dc = nullptr, *dp = nullptr;
    const bool small = n <= SMALL_LOOKUP;
    if (small) {
        if (!m->d_small.get()) TSX_TRY(m->d_small.alloc(SMALL_LOOKUP * (4 + 2) * 8));
        dk = m->d_small.get(); dc = dk + SMALL_LOOKUP * 4; dp = dc + SMALL_LOOKUP;
    } else {
        TSX_TRY(big_k.alloc(kb));
        if (big_c.alloc(n * 16) != TSX_HIP_OK) return TSX_HIP_ENOMEM;
        dk = big_k.get(); dc = big_c.get(); dp = dc + n;
    }
    const hipStream_t st = m->stream.get();
    auto run = [&]() -> int {
        if (hipMemcpyAsync(dk, kmers, kb, hipMemcpyHostToDevice, st) != hipSuccess) return TSX_HIP_EHIP;
        const int grid = grid_for(m, n, 8);
        DISPATCH_CANON(m, DISPATCH_WK(m, hipLaunchKernelGGL((get_counts_kernel<WKV, CANV>), dim3(grid), dim3(NT), 0, st,
                                                            m->p, (const uint64_t *)dk, (uint64_t)n, dc,
                                                            slots_out ? dp : (uint64_t *)nullptr)));
        if (hipGetLastError() != hipSuccess) return TSX_HIP_EHIP;
        if (hipMemcpyAsync(counts_out, dc, n * 8, hipMemcpyDeviceToHost, st) != hipSuccess) return TSX_HIP_EHIP;
        if (slots_out && hipMemcpyAsync(slots_out, dp, n * 8, hipMemcpyDeviceToHost, st) != hipSuccess) return TSX_HIP_EHIP;
        return hipStreamSynchronize(st) == hipSuccess ? TSX_HIP_OK : TSX_HIP_EHIP;
    };
    const int rc = run();
    if (!small) (void)hipStreamSynchronize(st);   // nothing queued may outlive the buffers of this call
    return rc;
}

extern "C" int tsx_hip_lookup_host(tsx_hip_map *m, const uint64_t *kmers, size_t n, uint64_t *counts_out,
                                   uint64_t *slots_out) {
    if (!slots_out && n) return TSX_HIP_EINVAL;
    return lookup_host(m, kmers, n, counts_out, slots_out);
}

extern "C" int tsx_hip_kmer_starts_host(tsx_hip_map *m, uint8_t *bits_out, size_t nbytes) {
    if (!m || !bits_out || nbytes * 8 < m->lay.slots) return TSX_HIP_EINVAL;
    HIP_TRY(hipSetDevice(m->device));
    const uint64_t nb = (m->lay.slots + 7) / 8;
    join_foreign(m, false);
    int rcz = ensure_zeroed(m, m->stream.get());
    if (rcz != TSX_HIP_OK) return rcz;
    DevBuf<uint8_t> d;
    TSX_TRY(d.alloc(nb));
    hipLaunchKernelGGL(kmer_starts_kernel, dim3(grid_for(m, nb, 8)), dim3(NT), 0, m->stream.get(), m->p, d.get(), nb);
    int rc = (hipGetLastError() == hipSuccess &&
              hipMemcpyAsync(bits_out, d.get(), nb, hipMemcpyDeviceToHost, m->stream.get()) == hipSuccess &&
              hipStreamSynchronize(m->stream.get()) == hipSuccess) ? TSX_HIP_OK : TSX_HIP_EHIP;
    if (rc == TSX_HIP_OK && nbytes > nb) memset(bits_out + nb, 0, nbytes - nb);
    return rc;
}

extern "C" int tsx_hip_get_counts_host(tsx_hip_map *m, const uint64_t *kmers, size_t n, uint64_t *counts_out) {
    return lookup_host(m, kmers, n, counts_out, nullptr);
}

// Words 0-2: the owners alive in this process (tsx_own.h) -- device buffers, pinned buffers, events + streams; tests
// take differences.  Word 7: entries of the deferred list of the last partitioned pass.  Words 3 and 4: the tiles the
// count launches of the map's last normalization covered, and those of them the record gate skipped.  Words 5-6 are
// spare and read 0.  Not part of include/tsxcount_hip.h.
extern "C" int tsx_hip_debug_counters(tsx_hip_map *m, uint64_t *out8) {
    if (!m || !out8) return TSX_HIP_EINVAL;
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipStreamSynchronize(m->stream.get()));
    for (int i = 0; i < 8; ++i) out8[i] = 0;
    out8[0] = (uint64_t)g_live_dev.load(); out8[1] = (uint64_t)g_live_pin.load(); out8[2] = (uint64_t)g_live_sync.load();
    out8[3] = m->norm_tiles; out8[4] = m->norm_skipped;
    if (m->d_def_n.get()) {
        unsigned long long dn = 0;
        HIP_TRY(hipMemcpy(&dn, m->d_def_n.get(), 8, hipMemcpyDeviceToHost));
        out8[7] = dn;
    }
    return TSX_HIP_OK;
}

extern "C" int tsx_hip_get_stats(tsx_hip_map *m, tsx_hip_stats *out) {
    if (!m || !out) return TSX_HIP_EINVAL;
    HIP_TRY(hipSetDevice(m->device));
    join_foreign(m, false);
    int rcz = ensure_zeroed(m, m->stream.get());
    if (rcz != TSX_HIP_OK) return rcz;
    HIP_TRY(hipMemsetAsync(m->p.stats + ST_SCRATCH, 0, 2 * sizeof(unsigned long long), m->stream.get()));
    HIP_TRY(hipMemsetAsync(m->p.stats + ST_SCRATCH3, 0, sizeof(unsigned long long), m->stream.get()));
    const int grid = grid_for(m, m->lay.slots, 8);
    hipLaunchKernelGGL(occupied_kernel, dim3(grid), dim3(NT), 0, m->stream.get(), m->p);
    HIP_TRY(hipGetLastError());
    unsigned long long st[ST_N];
    int rc = read_stats(m, st);
    if (rc != TSX_HIP_OK) return rc;
    out->kmers_added = st[ST_KMERS];
    out->insert_failures = st[ST_FAIL];
    out->overflow_carries = st[ST_CARRY];
    out->overflow_failures = st[ST_SECFAIL];
    out->lock_timeouts = st[ST_LOCKTO];
    out->fallback_inserts = st[ST_FALLBACK];
    out->distinct = st[ST_SCRATCH];
    out->overflow_used = st[ST_SCRATCH2];
    out->count_sum = st[ST_SCRATCH3];
    return TSX_HIP_OK;
}

// Entries of the table slots [slot_lo, slot_hi), grouped by owner rank (nranks = 1: plain dump).
static int dump_slots(tsx_hip_map *m, int nranks, uint64_t slot_lo, uint64_t slot_hi, void *dev_kmers_out,
                      void *dev_counts_out, size_t cap, void *dev_seg_counts, void *stream) {
    if (!m || nranks < 1 || nranks > 64 || !dev_kmers_out || !dev_counts_out || !dev_seg_counts) return TSX_HIP_EINVAL;
    if (slot_lo > slot_hi || slot_hi > m->lay.slots) return TSX_HIP_EINVAL;
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t st = pick_stream(m, stream);
    int rcz = ensure_zeroed(m, st);
    if (rcz != TSX_HIP_OK) return rcz;
    const int grid = grid_for(m, std::max<uint64_t>(1, slot_hi - slot_lo), 8);
    unsigned long long *seg = m->d_seg.get();
    HIP_TRY(hipMemsetAsync(seg, 0, 64 * sizeof(unsigned long long), st));
    DISPATCH_CANON(m, DISPATCH_WK(m, hipLaunchKernelGGL((dump_kernel<WKV, CANV>), dim3(grid), dim3(NT), 0, st, m->p, nranks, 0,
                                                        (uint64_t *)nullptr, (uint64_t *)nullptr, (uint64_t)0, seg, slot_lo,
                                                        slot_hi)));
    // segment sizes -> caller; exclusive prefix -> cursors (tiny: done on the host)
    unsigned long long h_seg[64];
    HIP_TRY(hipMemcpyAsync(h_seg, seg, 64 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    unsigned long long cur[64], total = 0;
    for (int r = 0; r < 64; ++r) { cur[r] = total; total += (r < nranks) ? h_seg[r] : 0; }
    if (total > cap) return TSX_HIP_ERANGE;
    HIP_TRY(hipMemcpyAsync(dev_seg_counts, h_seg, (size_t)nranks * sizeof(unsigned long long), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(seg, cur, 64 * sizeof(unsigned long long), hipMemcpyHostToDevice, st));
    DISPATCH_CANON(m, DISPATCH_WK(m, hipLaunchKernelGGL((dump_kernel<WKV, CANV>), dim3(grid), dim3(NT), 0, st, m->p, nranks, 1,
                                                        (uint64_t *)dev_kmers_out, (uint64_t *)dev_counts_out, (uint64_t)cap,
                                                        seg, slot_lo, slot_hi)));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));  // cur[] lives on this stack frame
    return TSX_HIP_OK;
}

extern "C" int tsx_hip_partition_device(tsx_hip_map *m, int nranks, void *dev_kmers_out, void *dev_counts_out,
                                        size_t cap, void *dev_seg_counts, void *stream) {
    if (!m) return TSX_HIP_EINVAL;
    return dump_slots(m, nranks, 0, m->lay.slots, dev_kmers_out, dev_counts_out, cap, dev_seg_counts, stream);
}

extern "C" int tsx_hip_dump_device(tsx_hip_map *m, void *dev_kmers_out, void *dev_counts_out, size_t cap,
                                   void *dev_n, void *stream) {
    if (!m || !dev_n) return TSX_HIP_EINVAL;
    return dump_slots(m, 1, 0, m->lay.slots, dev_kmers_out, dev_counts_out, cap, dev_n, stream);
}

extern "C" int tsx_hip_dump_range_device(tsx_hip_map *m, uint64_t slot_lo, uint64_t slot_hi, void *dev_kmers_out,
                                         void *dev_counts_out, size_t cap, void *dev_n, void *stream) {
    if (!m || !dev_n) return TSX_HIP_EINVAL;
    return dump_slots(m, 1, slot_lo, slot_hi, dev_kmers_out, dev_counts_out, cap, dev_n, stream);
}

extern "C" int tsx_hip_dump_host(tsx_hip_map *m, uint64_t *kmers_out, uint64_t *counts_out, size_t cap,
                                 size_t *n_out) {
    if (!m || !kmers_out || !counts_out || !n_out) return TSX_HIP_EINVAL;
    tsx_hip_stats s;
    int rc = tsx_hip_get_stats(m, &s);
    if (rc != TSX_HIP_OK) return rc;
    if (s.distinct > cap) return TSX_HIP_ERANGE;
    *n_out = (size_t)s.distinct;
    if (s.distinct == 0) return TSX_HIP_OK;
    DevBuf<uint64_t> dk, dc, dn;
    const size_t kb = (size_t)s.distinct * m->p.wk * 8;
    TSX_TRY(dk.alloc(kb));
    if (dc.alloc(s.distinct * 8) != TSX_HIP_OK || dn.alloc(64) != TSX_HIP_OK) return TSX_HIP_ENOMEM;
    TSX_TRY(tsx_hip_dump_device(m, dk.get(), dc.get(), (size_t)s.distinct, dn.get(), nullptr));
    if (hipMemcpy(kmers_out, dk.get(), kb, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(counts_out, dc.get(), s.distinct * 8, hipMemcpyDeviceToHost) != hipSuccess)
        return TSX_HIP_EHIP;
    return TSX_HIP_OK;
}

// ---- output: abundance histogram and the .count text (tsx_output.h) -------------
static const size_t WRITE_CHUNK_DEFAULT = (size_t)256 << 20;   // text bytes per chunk of tsx_hip_write_counts_host
static inline size_t line_max(const tsx_hip_map *m) { return (size_t)m->p.k + 22; }   // bases, TAB, 20 digits, newline

static int histogram_launch(tsx_hip_map *m, uint64_t slot_lo, uint64_t slot_hi, size_t nbins, void *dev_hist, hipStream_t st) {
    HIP_TRY(hipMemsetAsync(dev_hist, 0, nbins * sizeof(unsigned long long), st));
    const uint64_t n = slot_hi - slot_lo, sslots = m->p.sec_mask + 1;
    uint64_t grid = (uint64_t)grid_for(m, std::max<uint64_t>(n / HIST_UNROLL, sslots), 8);
    // A workgroup's LDS bins are flushed as int32: bound what one workgroup visits (pass A + pass B) below 2^31.
    auto per_wg = [&](uint64_t g) {
        const uint64_t a = 64 * HIST_UNROLL * (NT / 64), b = NT;
        return (n + g * a - 1) / (g * a) * a + (sslots + g * b - 1) / (g * b) * b;
    };
    while (per_wg(grid) >= (1ULL << 31) && grid < (1ULL << 30)) grid *= 2;
    if (per_wg(grid) >= (1ULL << 31)) return TSX_HIP_EINVAL;
    hipLaunchKernelGGL(count_histogram_kernel, dim3((unsigned)grid), dim3(NT), 0, st, m->p, slot_lo, slot_hi, (uint64_t)nbins,
                       (unsigned long long *)dev_hist);
    HIP_TRY(hipGetLastError());
    return TSX_HIP_OK;
}

extern "C" int tsx_hip_histogram_device(tsx_hip_map *m, uint64_t slot_lo, uint64_t slot_hi, size_t nbins, void *dev_hist,
                                        void *stream) {
    if (!m || !dev_hist || nbins < 2 || slot_lo > slot_hi || slot_hi > m->lay.slots) return TSX_HIP_EINVAL;
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t st = pick_stream(m, stream);
    int rc = ensure_zeroed(m, st);
    if (rc != TSX_HIP_OK) return rc;
    return histogram_launch(m, slot_lo, slot_hi, nbins, dev_hist, st);
}

extern "C" int tsx_hip_histogram_host(tsx_hip_map *m, uint64_t *hist_out, size_t nbins) {
    if (!m || !hist_out || nbins < 2) return TSX_HIP_EINVAL;
    HIP_TRY(hipSetDevice(m->device));
    join_foreign(m, false);
    DevBuf<uint64_t> d;
    TSX_TRY(d.alloc(nbins * sizeof(uint64_t)));
    TSX_TRY(tsx_hip_histogram_device(m, 0, m->lay.slots, nbins, d.get(), nullptr));
    if (hipMemcpyAsync(hist_out, d.get(), nbins * sizeof(uint64_t), hipMemcpyDeviceToHost, m->stream.get()) != hipSuccess ||
        hipStreamSynchronize(m->stream.get()) != hipSuccess)
        return TSX_HIP_EHIP;
    return TSX_HIP_OK;
}

// Zero the two counters and queue format_counts_kernel over [slot_lo, slot_hi) (nothing to format: counters only).
static int format_launch(tsx_hip_map *m, uint64_t slot_lo, uint64_t slot_hi, uint64_t lower, uint64_t upper, void *dev_text,
                         size_t cap, unsigned long long *d_nbytes, unsigned long long *d_nlines, hipStream_t st) {
    HIP_TRY(hipMemsetAsync(d_nbytes, 0, sizeof(unsigned long long), st));
    HIP_TRY(hipMemsetAsync(d_nlines, 0, sizeof(unsigned long long), st));
    if (slot_hi == slot_lo) return TSX_HIP_OK;
    const int grid = grid_for(m, slot_hi - slot_lo, 8);
    DISPATCH_CANON(m, DISPATCH_WK(m, hipLaunchKernelGGL((format_counts_kernel<WKV, CANV>), dim3(grid), dim3(NT), 0, st, m->p,
                                                        slot_lo, slot_hi, lower, upper, (uint8_t *)dev_text, (uint64_t)cap,
                                                        d_nbytes, d_nlines)));
    HIP_TRY(hipGetLastError());
    return TSX_HIP_OK;
}

extern "C" int tsx_hip_format_counts_device(tsx_hip_map *m, uint64_t slot_lo, uint64_t slot_hi, uint64_t lower, uint64_t upper,
                                            void *dev_text, size_t cap, void *dev_nbytes, void *dev_nlines, void *stream) {
    if (!m || !dev_nbytes || !dev_nlines || (!dev_text && cap) || lower > upper) return TSX_HIP_EINVAL;
    if (slot_lo > slot_hi || slot_hi > m->lay.slots) return TSX_HIP_EINVAL;
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t st = pick_stream(m, stream);
    int rc = ensure_zeroed(m, st);
    if (rc != TSX_HIP_OK) return rc;
    rc = format_launch(m, slot_lo, slot_hi, lower, upper, dev_text, cap, (unsigned long long *)dev_nbytes,
                       (unsigned long long *)dev_nlines, st);
    if (rc != TSX_HIP_OK) return rc;
    unsigned long long nb = 0;
    HIP_TRY(hipMemcpyAsync(&nb, dev_nbytes, sizeof nb, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return nb > cap ? TSX_HIP_ERANGE : TSX_HIP_OK;
}

// write(2) until every byte is out: short writes continue, EINTR retries, anything else is TSX_HIP_EIO.
static int write_all(int fd, const uint8_t *p, size_t n) {
    while (n) {
        const ssize_t w = write(fd, p, n);
        if (w < 0 && errno == EINTR) continue;
        if (w <= 0) {
            g_last_error = std::string("write: ") + (w < 0 ? strerror(errno) : "no progress");
            return TSX_HIP_EIO;
        }
        p += w;
        n -= (size_t)w;
    }
    return TSX_HIP_OK;
}

// The table written in chunks of `per` slots, one chunk ahead: the device makes chunk i + 1 while the host writes chunk i.
// Two device and two pinned payload buffers (the second pair only when a second chunk exists), the device words a chunk's
// making needs (its two result words among them) and the pinned mirror of those two.  Stream order:
//   make(0) res(0) | payload(0) make(1) res(1) | payload(1) make(2) res(2) | ...
struct ChunkAhead {
    struct Range { size_t at, n; };   // bytes of a payload buffer
    const uint64_t slots, per;
    DevBuf<uint8_t> dev[2];
    PinBuf<uint8_t> host[2];
    DevBuf<unsigned long long> dev_res;
    PinBuf<unsigned long long> host_res;
    Event res_ready, payload_ready;
    SyncAtExit wait;   // nothing queued may outlive the buffers
    ChunkAhead(hipStream_t st, uint64_t slots_, uint64_t per_) : slots(slots_), per(per_), wait(st) {}

    int init(size_t buf, size_t dev_words) {
        if (dev_res.alloc(dev_words * 8) != TSX_HIP_OK || host_res.alloc(2 * 8) != TSX_HIP_OK) return TSX_HIP_ENOMEM;
        for (int b = 0; b < (slots > per ? 2 : 1); ++b)
            if (dev[b].alloc(buf) != TSX_HIP_OK || host[b].alloc(buf) != TSX_HIP_OK) return TSX_HIP_ENOMEM;
        if (res_ready.create() != TSX_HIP_OK || payload_ready.create() != TSX_HIP_OK) return TSX_HIP_EHIP;
        return TSX_HIP_OK;
    }
    // For the chunk of slots [lo, hi), each returning a TSX_HIP_* code (the first that is not OK ends the run and is returned):
    // make(lo, hi, payload, words, mirror)  queues it into the device payload buffer and its two result words into the mirror
    // fetch(lo, hi, res, ranges)            checks its result words and names the (at most two) ranges to copy back
    // emit(lo, hi, res, payload, ranges)    writes it from the host payload buffer, once the copy has landed
    template <typename Make, typename Fetch, typename Emit>
    int run(Make make, Fetch fetch, Emit emit) {
        const hipStream_t st = wait.st;
        auto queue = [&](uint64_t lo, uint8_t *payload) -> int {
            TSX_TRY(make(lo, std::min(slots, lo + per), payload, dev_res.get(), host_res.get()));
            HIP_TRY(hipEventRecord(res_ready.get(), st));
            return TSX_HIP_OK;
        };
        TSX_TRY(queue(0, dev[0].get()));
        for (uint64_t lo = 0, b = 0; lo < slots; lo += per, b ^= 1) {
            const uint64_t hi = std::min(slots, lo + per);
            HIP_TRY(hipEventSynchronize(res_ready.get()));
            const unsigned long long res[2] = {host_res.get()[0], host_res.get()[1]};   // (the next chunk's overwrite the mirror)
            Range r[2] = {{0, 0}, {0, 0}};
            TSX_TRY(fetch(lo, hi, res, r));
            for (const Range &x : r)
                if (x.n) HIP_TRY(hipMemcpyAsync(host[b].get() + x.at, dev[b].get() + x.at, x.n, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipEventRecord(payload_ready.get(), st));
            if (hi < slots) TSX_TRY(queue(hi, dev[b ^ 1].get()));
            HIP_TRY(hipEventSynchronize(payload_ready.get()));
            TSX_TRY(emit(lo, hi, res, host[b].get(), r));
        }
        return TSX_HIP_OK;
    }
};

// The table as text: a chunk is floor(chunk_bytes / line_max) slots, so its text always fits.
extern "C" int tsx_hip_write_counts_host(tsx_hip_map *m, int fd, uint64_t lower, uint64_t upper, size_t chunk_bytes,
                                         uint64_t *lines_out, uint64_t *bytes_out) {
    if (lines_out) *lines_out = 0;
    if (bytes_out) *bytes_out = 0;
    if (!m || fd < 0 || lower > upper || (chunk_bytes && chunk_bytes < line_max(m))) return TSX_HIP_EINVAL;
    if (!chunk_bytes) chunk_bytes = WRITE_CHUNK_DEFAULT;
    const uint64_t slots = m->lay.slots, per = chunk_bytes / line_max(m);
    const size_t buf = (size_t)std::min<uint64_t>(per, slots) * line_max(m);
    HIP_TRY(hipSetDevice(m->device));
    join_foreign(m, false);
    hipStream_t st = m->stream.get();
    TSX_TRY(ensure_zeroed(m, st));
    ChunkAhead ahead(st, slots, per);
    TSX_TRY(ahead.init(buf, 2));
    uint64_t lines = 0, bytes = 0;
    const int rc = ahead.run(
        [&](uint64_t lo, uint64_t hi, uint8_t *d_text, unsigned long long *d_cnt, unsigned long long *h_cnt) -> int {
            TSX_TRY(format_launch(m, lo, hi, lower, upper, d_text, buf, d_cnt, d_cnt + 1, st));
            HIP_TRY(hipMemcpyAsync(h_cnt, d_cnt, 2 * 8, hipMemcpyDeviceToHost, st));
            return TSX_HIP_OK;
        },
        [&](uint64_t, uint64_t, const unsigned long long *cnt, ChunkAhead::Range *r) -> int {   // cnt: bytes, lines
            if (cnt[0] > buf) return TSX_HIP_ERANGE;   // cannot happen: a chunk's text fits by construction
            r[0].n = (size_t)cnt[0];
            return TSX_HIP_OK;
        },
        [&](uint64_t, uint64_t, const unsigned long long *cnt, const uint8_t *text, const ChunkAhead::Range *) -> int {
            TSX_TRY(write_all(fd, text, (size_t)cnt[0]));
            bytes += cnt[0]; lines += cnt[1];
            return TSX_HIP_OK;
        });
    if (lines_out) *lines_out = lines;
    if (bytes_out) *bytes_out = bytes;
    return rc;
}

// ---- k-mer database: save, load, merge (tsx_db.h; DESIGN.md §3 "K-mer database") -------------------------------
static const uint8_t DB_MAGIC[8] = {'T', 'S', 'X', 'K', 'M', 'E', 'R', 'S'};
static const uint32_t DB_VERSION = 1;
static const size_t DB_HEADER = 128, DB_CHUNK_HEAD = 32;
static const size_t DB_CHUNK_DEFAULT = (size_t)256 << 20;
static_assert(__BYTE_ORDER__ == __ORDER_LITTLE_ENDIAN__, "the database format is little-endian, as the host");

// FNV-1a, 64 bit: the checksum of the header (bytes 0 .. 119) and of the carry section.
static uint64_t db_fnv(const void *p, size_t n, uint64_t h = 0xCBF29CE484222325ULL) {
    const uint8_t *b = (const uint8_t *)p;
    for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 0x100000001B3ULL; }
    return h;
}
template <typename T> static inline void db_put(uint8_t *b, size_t at, T v) { memcpy(b + at, &v, sizeof v); }
template <typename T> static inline T db_get(const uint8_t *b, size_t at) { T v; memcpy(&v, b + at, sizeof v); return v; }

static int db_fail(const std::string &why) { g_last_error = why; return TSX_HIP_EFORMAT; }

static void db_header_bytes(const tsx_hip_db_info &in, uint64_t carry_sum, uint8_t *b) {
    memset(b, 0, DB_HEADER);
    memcpy(b, DB_MAGIC, 8);
    db_put<uint32_t>(b, 8, in.version); db_put<uint32_t>(b, 12, (uint32_t)DB_HEADER);
    db_put<int32_t>(b, 16, in.k); db_put<int32_t>(b, 20, in.l); db_put<int32_t>(b, 24, in.entry_limbs);
    db_put<int32_t>(b, 28, in.func_bits); db_put<int32_t>(b, 32, in.reprobe_bits); db_put<int32_t>(b, 36, in.count_bits);
    db_put<int32_t>(b, 40, in.seg_bits); db_put<int32_t>(b, 44, in.overflow_l); db_put<uint64_t>(b, 48, in.hash_seed);
    db_put<int32_t>(b, 56, in.canonical); db_put<int32_t>(b, 60, in.acgt_only); db_put<int32_t>(b, 64, in.min_qual_char);
    db_put<uint64_t>(b, 72, in.kmers_added); db_put<uint64_t>(b, 80, in.distinct); db_put<uint64_t>(b, 88, in.count_sum);
    db_put<uint64_t>(b, 96, in.carry_records); db_put<uint64_t>(b, 104, carry_sum);
    db_put<uint64_t>(b, 120, db_fnv(b, 120));
}

static int db_parse_header(const uint8_t *b, tsx_hip_db_info *out, uint64_t *carry_sum) {
    if (memcmp(b, DB_MAGIC, 8) != 0) return db_fail("not a k-mer database (bad magic)");
    tsx_hip_db_info d;
    d.version = db_get<uint32_t>(b, 8);
    if (d.version != DB_VERSION || db_get<uint32_t>(b, 12) != DB_HEADER)
        return db_fail("k-mer database format version " + std::to_string(d.version) + " (this library reads version 1)");
    if (db_get<uint64_t>(b, 120) != db_fnv(b, 120)) return db_fail("k-mer database header checksum mismatch");
    d.k = db_get<int32_t>(b, 16); d.l = db_get<int32_t>(b, 20); d.entry_limbs = db_get<int32_t>(b, 24);
    d.func_bits = db_get<int32_t>(b, 28); d.reprobe_bits = db_get<int32_t>(b, 32); d.count_bits = db_get<int32_t>(b, 36);
    d.seg_bits = db_get<int32_t>(b, 40); d.overflow_l = db_get<int32_t>(b, 44); d.hash_seed = db_get<uint64_t>(b, 48);
    d.canonical = db_get<int32_t>(b, 56); d.acgt_only = db_get<int32_t>(b, 60); d.min_qual_char = db_get<int32_t>(b, 64);
    d.kmers_added = db_get<uint64_t>(b, 72); d.distinct = db_get<uint64_t>(b, 80); d.count_sum = db_get<uint64_t>(b, 88);
    d.carry_records = db_get<uint64_t>(b, 96);
    if (d.k < 1 || d.k > 127 || d.l < 4 || d.l > 36 || d.entry_limbs < 1 || d.entry_limbs > 4 || d.seg_bits < 1 ||
        d.seg_bits > d.l || (d.canonical & ~1) || (d.acgt_only & ~1) || d.min_qual_char < 0 || d.min_qual_char > 255 ||
        d.carry_records > ((uint64_t)1 << d.l))
        return db_fail("k-mer database header out of range");
    if (out) *out = d;
    if (carry_sum) *carry_sum = db_get<uint64_t>(b, 104);
    return TSX_HIP_OK;
}

// read(2) -- or, with at >= 0, pread(2) from that offset, which leaves the file position alone -- until n bytes are in: a
// file that ends before is EFORMAT ("truncated (<what>)"), an error of the call EIO (g_last_error says which).
static int db_read_exact(int fd, void *p, size_t n, const char *what, off_t at = -1) {
    size_t got = 0;
    while (got < n) {
        const ssize_t r = at < 0 ? read(fd, (uint8_t *)p + got, n - got) : pread(fd, (uint8_t *)p + got, n - got, at + (off_t)got);
        if (r < 0 && errno == EINTR) continue;
        if (r < 0) { g_last_error = std::string(at < 0 ? "read: " : "pread: ") + strerror(errno); return TSX_HIP_EIO; }
        if (r == 0) return db_fail(std::string("k-mer database truncated (") + what + ")");
        got += (size_t)r;
    }
    return TSX_HIP_OK;
}

extern "C" int tsx_hip_db_read_info(int fd, tsx_hip_db_info *out) {
    if (fd < 0 || !out) return TSX_HIP_EINVAL;
    uint8_t b[DB_HEADER];
    TSX_TRY(db_read_exact(fd, b, DB_HEADER, "header", 0));
    return db_parse_header(b, out, nullptr);
}

// Slots per chunk such that a chunk's worst case (every slot occupied) fits chunk_bytes; 0 when not even 64 do.
static uint64_t db_span(size_t chunk_bytes, int W) {
    if (chunk_bytes < DB_CHUNK_HEAD) return 0;
    return (uint64_t)((chunk_bytes - DB_CHUNK_HEAD) / (8 + 64 * 8 * (size_t)W)) * 64;
}
static inline uint64_t db_tiles(uint64_t lo, uint64_t hi) { return (hi - lo + DB_TILE - 1) / DB_TILE; }

// The n carry records of the secondary array, sorted by slot (the file does not depend on the array's probe order).
static int db_gather_carry(tsx_hip_map *m, uint64_t n, std::vector<uint64_t> &carry) {
    const int RW = 2 + m->p.W;
    carry.assign((size_t)n * RW, 0);
    if (!n) return TSX_HIP_OK;
    hipStream_t st = m->stream.get();
    DevBuf<uint64_t> rec;
    SyncAtExit wait(st);
    TSX_TRY(rec.alloc(carry.size() * 8 + 8));
    uint64_t *const d_rec = rec.get();
    unsigned long long *const d_n = (unsigned long long *)(d_rec + carry.size());
    unsigned long long h_n = 0;
    HIP_TRY(hipMemsetAsync(d_n, 0, 8, st));
    hipLaunchKernelGGL(db_carry_gather_kernel, dim3(grid_for(m, m->p.sec_mask + 1, 8)), dim3(NT), 0, st, m->p, d_rec, n, d_n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(carry.data(), d_rec, carry.size() * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&h_n, d_n, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (h_n != n) { g_last_error = "secondary array changed during the save"; return TSX_HIP_EHIP; }
    std::vector<uint64_t> order(n), sorted(carry.size());
    for (uint64_t i = 0; i < n; ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) { return carry[a * RW] < carry[b * RW]; });
    for (uint64_t i = 0; i < n; ++i) memcpy(&sorted[i * RW], &carry[order[i] * RW], (size_t)RW * 8);
    carry.swap(sorted);
    return TSX_HIP_OK;
}

// What the header says of a map and its stats.
static tsx_hip_db_info db_info_of(const tsx_hip_map *m, const tsx_hip_stats &s) {
    tsx_hip_db_info info;
    memset(&info, 0, sizeof info);
    info.version = DB_VERSION; info.k = m->p.k; info.l = m->p.l; info.entry_limbs = m->p.W; info.func_bits = m->p.F;
    info.reprobe_bits = m->p.R; info.count_bits = m->p.C; info.seg_bits = m->p.S; info.overflow_l = m->lay.overflow_l;
    info.canonical = m->canon ? 1 : 0; info.acgt_only = m->p.acgt_only ? 1 : 0; info.min_qual_char = (int32_t)m->minq;
    info.hash_seed = m->seed; info.kmers_added = s.kmers_added; info.distinct = s.distinct; info.count_sum = s.count_sum;
    info.carry_records = s.overflow_used;
    return info;
}

// The chunks of span slots each: head, bitmap, entries.  A payload buffer holds the bitmap of a full span, then the entries.
static int db_write_chunks(tsx_hip_map *m, int fd, uint64_t span, uint64_t &entries, uint64_t &bytes) {
    const int W = m->p.W;
    const uint64_t ntmax = db_tiles(0, span);
    hipStream_t st = m->stream.get();
    ChunkAhead ahead(st, m->lay.slots, span);
    TSX_TRY(ahead.init((size_t)(span / 64 + span * W) * 8, ntmax + 2));   // (device words: tile offsets, then the checksum)
    return ahead.run(
        [&](uint64_t lo, uint64_t hi, uint8_t *d_buf, unsigned long long *d_tile, unsigned long long *h_res) -> int {
            const uint64_t nt = db_tiles(lo, hi);
            uint64_t *bm = (uint64_t *)d_buf, *ent = bm + span / 64;
            unsigned long long *const d_sum = d_tile + ntmax + 1;
            HIP_TRY(hipMemsetAsync(d_sum, 0, 8, st));
            hipLaunchKernelGGL(db_count_table_kernel, dim3((unsigned)nt), dim3(NT), 0, st, m->p, lo, hi, d_tile);
            hipLaunchKernelGGL(db_scan_kernel, dim3(1), dim3(NT), 0, st, d_tile, nt);
            hipLaunchKernelGGL(db_pack_kernel, dim3((unsigned)nt), dim3(NT), 0, st, m->p, lo, hi, (const unsigned long long *)d_tile,
                               bm, ent, span, d_sum);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(h_res, d_tile + nt, 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(h_res + 1, d_sum, 8, hipMemcpyDeviceToHost, st));
            return TSX_HIP_OK;
        },
        [&](uint64_t lo, uint64_t hi, const unsigned long long *res, ChunkAhead::Range *r) -> int {   // res: entries, checksum
            if (res[0] > hi - lo) return TSX_HIP_ERANGE;   // cannot happen: a tile counts at most its slots
            r[0] = {0, (size_t)((hi - lo + 63) / 64) * 8};
            r[1] = {(size_t)(span / 64) * 8, (size_t)res[0] * W * 8};
            return TSX_HIP_OK;
        },
        [&](uint64_t lo, uint64_t hi, const unsigned long long *res, const uint8_t *h_buf, const ChunkAhead::Range *r) -> int {
            const uint64_t ch[4] = {lo, hi, res[0], res[1]};
            TSX_TRY(write_all(fd, (const uint8_t *)ch, DB_CHUNK_HEAD));
            TSX_TRY(write_all(fd, h_buf + r[0].at, r[0].n));
            TSX_TRY(write_all(fd, h_buf + r[1].at, r[1].n));
            bytes += DB_CHUNK_HEAD + r[0].n + r[1].n;
            entries += res[0];
            return TSX_HIP_OK;
        });
}

extern "C" int tsx_hip_save_host(tsx_hip_map *m, int fd, size_t chunk_bytes, uint64_t *entries_out, uint64_t *bytes_out) {
    if (entries_out) *entries_out = 0;
    if (bytes_out) *bytes_out = 0;
    if (!m || fd < 0) return TSX_HIP_EINVAL;
    if (m->p.lg != m->p.l) { g_last_error = "a shard of a multi-GPU table is not saved"; return TSX_HIP_EINVAL; }
    if (!chunk_bytes) chunk_bytes = DB_CHUNK_DEFAULT;
    const uint64_t slots = m->lay.slots;
    const uint64_t span = std::min<uint64_t>(db_span(chunk_bytes, m->p.W), (slots + 63) & ~63ULL);
    if (span == 0) return TSX_HIP_EINVAL;
    tsx_hip_stats s;
    TSX_TRY(tsx_hip_get_stats(m, &s));   // (zeroes a lazily cleared table; waits for everything queued)
    std::vector<uint64_t> carry;
    TSX_TRY(db_gather_carry(m, s.overflow_used, carry));
    uint8_t head[DB_HEADER];
    db_header_bytes(db_info_of(m, s), db_fnv(carry.data(), carry.size() * 8), head);
    TSX_TRY(write_all(fd, head, DB_HEADER));
    TSX_TRY(write_all(fd, (const uint8_t *)carry.data(), carry.size() * 8));
    uint64_t bytes = DB_HEADER + carry.size() * 8, entries = 0;
    int rc = db_write_chunks(m, fd, span, entries, bytes);
    if (rc == TSX_HIP_OK) {
        const uint64_t end[4] = {slots, slots, 0, 0};
        rc = write_all(fd, (const uint8_t *)end, DB_CHUNK_HEAD);
        if (rc == TSX_HIP_OK) bytes += DB_CHUNK_HEAD;
    }
    if (rc == TSX_HIP_OK && entries != s.distinct) { g_last_error = "the table changed during the save"; rc = TSX_HIP_EHIP; }
    if (entries_out) *entries_out = entries;
    if (bytes_out) *bytes_out = bytes;
    return rc;
}

// Staging of one chunk of the load (two of them alternate): the file bytes in pinned memory and on the device, the tile
// offsets, the k-mers and counts of the re-insert path, and the result words of the load kernels.
struct DbStage {
    PinBuf<uint8_t> h;
    DevBuf<uint8_t> d;
    DevBuf<unsigned long long> d_tile;
    DevBuf<uint64_t> d_kx;                            // kmers (WK words) then counts, per entry
    DevBuf<unsigned long long> d_res;
    PinBuf<unsigned long long> h_res;
    Event done;
    bool busy = false;
    uint64_t n = 0, sum = 0;                          // what the chunk's head promised
    uint64_t zero_carried = 0;                        // its entries with in-slot count 0 that a carry record names
};

// The database layout as TableParams (what words_to_kmer needs), with its inverse mapping uploaded to *d_ilut.
static int db_source_params(const tsx_hip_db_info &d, TableParams &sp, DevBuf<uint64_t> *d_ilut) {
    tsx_hip_map src;   // host fields only: no device allocations
    if (derive_layout(&src, d.k, d.l, d.count_bits, d.overflow_l, 0, 0) != TSX_HIP_OK || src.p.W != d.entry_limbs ||
        src.p.F != d.func_bits || src.p.R != d.reprobe_bits || src.p.C != d.count_bits)
        return db_fail("k-mer database header: inconsistent slot layout");
    src.p.S = d.seg_bits;
    src.p.seg_mask = (1ULL << d.seg_bits) - 1ULL;
    src.seed = d.hash_seed;
    if (d_ilut) {
        int rc = make_mapping(&src);
        if (rc != TSX_HIP_OK) return rc;
        make_lut(&src, src.irows, src.ilut);
        TSX_TRY(d_ilut->alloc(src.ilut.size() * 8));
        HIP_TRY(hipMemcpy(d_ilut->get(), src.ilut.data(), src.ilut.size() * 8, hipMemcpyHostToDevice));
        src.p.ilut = d_ilut->get();
    }
    src.p.table = nullptr; src.p.sec_keys = src.p.sec_cnt = nullptr; src.p.stats = nullptr; src.p.lut = nullptr;
    src.p.roll = nullptr; src.p.seg_dirty = nullptr;
    sp = src.p;
    return TSX_HIP_OK;
}

// The header of the file at fd, and whether map m can take its k-mers at all.
static int db_read_header(const tsx_hip_map *m, int fd, tsx_hip_db_info *d, uint64_t *carry_sum) {
    uint8_t head[DB_HEADER];
    TSX_TRY(db_read_exact(fd, head, DB_HEADER, "header"));
    TSX_TRY(db_parse_header(head, d, carry_sum));
    if (d->k != m->p.k || d->canonical != (m->canon ? 1 : 0) || d->acgt_only != (m->p.acgt_only ? 1 : 0) ||
        d->min_qual_char != (int)m->minq) {
        g_last_error = "the database was counted with a different k, canonical mode or base rule than this table";
        return TSX_HIP_EINVAL;
    }
    return TSX_HIP_OK;
}

// Host only: the carry records from *next on with a slot below hi (they are sorted by slot, so a chunk's come in order)
// against chunk [lo, hi) of n entries, hbm its bitmap and hent its entries of W words.  Slot pos must be occupied and hold
// the record's words; a popcount of the bitmap up to pos gives the entry's index.  In-slot counts of 0 are counted into
// *zero_carried and compared with the device's count of them (DbLoad::finish), so that no entry's total count is 0.
static int db_match_carry(const uint64_t *rec, uint64_t nrec, uint64_t *next, int W, int cshift, uint64_t lo, uint64_t hi,
                          uint64_t n, const uint64_t *hbm, const uint64_t *hent, uint64_t *zero_carried) {
    const int RW = 2 + W;
    uint64_t w = 0, before = 0;   // set bits of the words before w
    *zero_carried = 0;
    for (; *next < nrec && rec[*next * RW] < hi; ++*next) {
        const uint64_t *r = &rec[*next * RW];
        const uint64_t off = r[0] - lo, wc = off >> 6;
        for (; w < wc; ++w) before += (uint64_t)__builtin_popcountll(hbm[w]);
        const uint64_t bit = 1ULL << (off & 63);
        const uint64_t idx = before + (uint64_t)__builtin_popcountll(hbm[wc] & (bit - 1ULL));
        if (!(hbm[wc] & bit) || idx >= n || memcmp(&hent[idx * W], r + 2, (size_t)W * 8) != 0)
            return db_fail("k-mer database: a carry record does not match the entry at its slot");
        *zero_carried += (hent[idx * W] >> cshift) == 0 ? 1 : 0;
    }
    return TSX_HIP_OK;
}

// One load, step by step (tsx_hip_load_host calls them in order).  A step that fails returns at once: the stages left
// busy are waited for (the wait is declared behind every owner), not inspected.  The map is left as the steps before
// left it -- used, not fresh, a table placed in part -- and clear recovers it.
struct DbLoad {
    tsx_hip_map *const m;
    const int fd;
    const tsx_hip_db_info d;
    const uint64_t carry_sum;
    const size_t chunk_bytes;
    const hipStream_t st;
    // placed as it is, slot by slot: an empty table of the database's geometry and seed.  Else every k-mer is re-inserted.
    const bool direct;
    const int W, RW, WK;
    const uint64_t slots;
    TableParams sp;                      // the database's layout (the table's own when direct)
    unsigned long long kmers_before = 0;
    std::vector<uint64_t> rec;           // the carry records: each is checked against the chunk that holds its pos
    uint64_t next_carry = 0, expect_lo = 0, entries = 0;
    DevBuf<uint64_t> d_ilut, carry;
    DbStage sg[2];
    SyncAtExit wait;

    DbLoad(tsx_hip_map *m_, int fd_, const tsx_hip_db_info &d_, uint64_t carry_sum_, size_t chunk_bytes_)
        : m(m_), fd(fd_), d(d_), carry_sum(carry_sum_), chunk_bytes(chunk_bytes_), st(m_->stream.get()),
          direct(!m_->used && d_.l == m_->p.l && d_.entry_limbs == m_->p.W && d_.func_bits == m_->p.F &&
                 d_.reprobe_bits == m_->p.R && d_.count_bits == m_->p.C && d_.seg_bits == m_->p.S && d_.hash_seed == m_->seed),
          W(d_.entry_limbs), RW(2 + d_.entry_limbs), WK(m_->p.wk), slots(1ULL << d_.l), wait(m_->stream.get()) {}

    int begin() {
        TSX_TRY(db_source_params(d, sp, direct ? nullptr : &d_ilut));
        // the table: a direct load writes every slot, so a lazily cleared table needs no memset
        if (direct) { sp = m->p; m->fresh = false; }
        else TSX_TRY(ensure_zeroed(m, st));
        m->used = true;
        HIP_TRY(hipMemcpyAsync(&kmers_before, m->p.stats + ST_KMERS, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return TSX_HIP_OK;
    }

    // Read, checksum, every record sane and the slots ascending; then uploaded and placed or re-inserted.
    int carry_section() {
        if (!d.carry_records) return TSX_HIP_OK;
        rec.resize((size_t)d.carry_records * RW);
        TSX_TRY(db_read_exact(fd, rec.data(), rec.size() * 8, "carry records"));
        if (db_fnv(rec.data(), rec.size() * 8) != carry_sum) return db_fail("k-mer database carry records checksum mismatch");
        for (uint64_t i = 0; i < d.carry_records; ++i) {
            const uint64_t *r = &rec[i * RW];
            const uint64_t rp = r[2] & ((1ULL << sp.R) - 1ULL);
            if (r[0] >= slots || r[1] == 0 || r[2] == 0 || rp == 0 || rp > sp.max_reprobes || (r[2] & sp.lock_bit))
                return db_fail("k-mer database: malformed carry record");
            if (i > 0 && r[0] <= r[-RW]) return db_fail("k-mer database: carry records not sorted by slot or not unique");
        }
        const size_t kx = direct ? 0 : (size_t)d.carry_records * (WK + 1);
        if (carry.alloc((rec.size() + kx) * 8) != TSX_HIP_OK) return TSX_HIP_ENOMEM;
        uint64_t *const d_carry = carry.get();
        HIP_TRY(hipMemcpyAsync(d_carry, rec.data(), rec.size() * 8, hipMemcpyHostToDevice, st));
        const int grid = grid_for(m, d.carry_records, 8);
        uint64_t *kx_k = d_carry + rec.size(), *kx_c = kx_k + (size_t)d.carry_records * WK;
        if (direct) {
            hipLaunchKernelGGL((db_carry_kernel<true, 1>), dim3(grid), dim3(NT), 0, st, m->p, sp, (const uint64_t *)d_carry,
                               (uint64_t)d.carry_records, (uint64_t *)nullptr, (uint64_t *)nullptr);
        } else {
            DISPATCH_WK(m, hipLaunchKernelGGL((db_carry_kernel<false, WKV>), dim3(grid), dim3(NT), 0, st, m->p, sp,
                                              (const uint64_t *)d_carry, (uint64_t)d.carry_records, kx_k, kx_c));
        }
        HIP_TRY(hipGetLastError());
        if (!direct) TSX_TRY(tsx_hip_add_kmers_device(m, kx_k, kx_c, (size_t)d.carry_records, nullptr));
        HIP_TRY(hipStreamSynchronize(st));
        return TSX_HIP_OK;
    }

    // The next chunk head ch = {lo, hi, entries, checksum}: the chunks tile the table in order, the end marker closes it.
    int chunk_head(uint64_t *ch) {
        TSX_TRY(db_read_exact(fd, ch, DB_CHUNK_HEAD, "no end marker"));
        const uint64_t lo = ch[0], hi = ch[1], n = ch[2];
        if (lo != expect_lo || hi > slots || (lo == hi && (lo != slots || n != 0)) || n > hi - lo || ((hi - lo) & 63 && hi != slots))
            return db_fail("k-mer database: chunks do not tile the table");
        expect_lo = hi;
        return TSX_HIP_OK;
    }

    // The chunk behind head ch into an idle stage: room for it, its bytes from the file, its carry records matched.
    int read_chunk(DbStage &s, const uint64_t *ch) {
        const uint64_t lo = ch[0], hi = ch[1], n = ch[2];
        const uint64_t nbm = (hi - lo + 63) / 64, nt = db_tiles(lo, hi);
        const size_t bytes = (size_t)(nbm + n * W) * 8;
        // grow-only; chunk_bytes is the first size.  (No wait: s.done has been waited for, nothing reads the stage.)
        const size_t want = std::max(bytes, std::min(chunk_bytes, (size_t)(slots / 64 + slots * W) * 8));
        if (bytes > s.d.cap()) s.h.reset();   // (both or none: d is allocated last)
        if (s.h.reserve(nullptr, bytes, want) != TSX_HIP_OK || s.d.reserve(nullptr, bytes, want) != TSX_HIP_OK) return TSX_HIP_ENOMEM;
        TSX_TRY(s.d_tile.reserve(nullptr, (nt + 1) * 8, (nt + 1) * 8));
        const size_t kxb = (size_t)std::max<uint64_t>(1, n) * (WK + 1) * 8;
        if (!direct) TSX_TRY(s.d_kx.reserve(nullptr, kxb, kxb));
        TSX_TRY(db_read_exact(fd, s.h.get(), bytes, "chunk"));
        s.n = n; s.sum = ch[3];
        const uint64_t *hbm = (const uint64_t *)s.h.get();
        return db_match_carry(rec.data(), d.carry_records, &next_carry, W, sp.cshift, lo, hi, n, hbm, hbm + nbm, &s.zero_carried);
    }

    // Queue the staged chunk [lo, hi): copy, entries per tile counted and scanned, entries placed or turned into k-mers
    // and re-inserted, the result words back.
    int queue_chunk(DbStage &s, uint64_t lo, uint64_t hi) {
        const uint64_t n = s.n, nbm = (hi - lo + 63) / 64, nt = db_tiles(lo, hi);
        const uint64_t *bm = (const uint64_t *)s.d.get(), *ent = bm + nbm;
        uint64_t *kx_k = s.d_kx.get(), *kx_c = kx_k ? kx_k + n * WK : nullptr;
        unsigned long long *const s_tile = s.d_tile.get(), *const s_res = s.d_res.get();
        const unsigned nb = (unsigned)((nt + NT / 64 - 1) / (NT / 64));
        HIP_TRY(hipMemcpyAsync(s.d.get(), s.h.get(), (size_t)(nbm + n * W) * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(s_res, 0, DB_RES_N * 8, st));
        hipLaunchKernelGGL(db_count_bitmap_kernel, dim3(nb), dim3(NT), 0, st, bm, nbm, nt, s_tile);
        hipLaunchKernelGGL(db_scan_kernel, dim3(1), dim3(NT), 0, st, s_tile, nt);
        if (direct) {
            hipLaunchKernelGGL((db_load_kernel<true, 1>), dim3((unsigned)nt), dim3(NT), 0, st, m->p, sp, lo, hi, bm, ent, n,
                               (const unsigned long long *)s_tile, (uint64_t *)nullptr, (uint64_t *)nullptr, s_res);
        } else {
            DISPATCH_WK(m, hipLaunchKernelGGL((db_load_kernel<false, WKV>), dim3((unsigned)nt), dim3(NT), 0, st, m->p, sp, lo, hi,
                                              bm, ent, n, (const unsigned long long *)s_tile, kx_k, kx_c, s_res));
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(s_res + DB_RES_TOTAL, s_tile + nt, 8, hipMemcpyDeviceToDevice, st));
        if (!direct && n) TSX_TRY(tsx_hip_add_kmers_device(m, kx_k, kx_c, (size_t)n, nullptr));
        HIP_TRY(hipMemcpyAsync(s.h_res.get(), s_res, DB_RES_N * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipEventRecord(s.done.get(), st));
        s.busy = true;
        return TSX_HIP_OK;
    }

    // The result of a chunk whose work has finished.
    int finish(DbStage &s) {
        s.busy = false;
        const unsigned long long *res = s.h_res.get();
        if (res[DB_RES_TOTAL] != s.n) return db_fail("k-mer database chunk: bitmap and entry count disagree");
        if (res[DB_RES_BAD]) return db_fail("k-mer database chunk: malformed entries");
        if (res[DB_RES_SUM] != s.sum) return db_fail("k-mer database chunk checksum mismatch");
        if (res[DB_RES_ZERO] != s.zero_carried) return db_fail("k-mer database chunk: an entry with count 0");
        entries += s.n;
        return TSX_HIP_OK;
    }

    // Chunk by chunk up to the end marker: the host reads chunk i + 1 while the device places chunk i.
    int chunks() {
        for (DbStage &s : sg)
            if (s.done.create() != TSX_HIP_OK || s.d_res.alloc(DB_RES_N * 8) != TSX_HIP_OK || s.h_res.alloc(DB_RES_N * 8) != TSX_HIP_OK)
                return TSX_HIP_ENOMEM;
        for (uint64_t i = 0;; ++i) {
            DbStage &s = sg[i & 1];
            if (s.busy) {
                HIP_TRY(hipEventSynchronize(s.done.get()));
                TSX_TRY(finish(s));
            }
            uint64_t ch[4];
            TSX_TRY(chunk_head(ch));
            if (ch[0] == slots) break;
            TSX_TRY(read_chunk(s, ch));
            TSX_TRY(queue_chunk(s, ch[0], ch[1]));
        }
        HIP_TRY(hipStreamSynchronize(st));
        for (DbStage &s : sg)
            if (s.busy) TSX_TRY(finish(s));
        return TSX_HIP_OK;
    }

    int end() {
        if (entries != d.distinct) return db_fail("k-mer database: entry count differs from the header");
        // kmers_added grows by the database's (the re-insert has added the sum of the counts instead)
        const unsigned long long ka = kmers_before + d.kmers_added;
        HIP_TRY(hipMemcpyAsync(m->p.stats + ST_KMERS, &ka, 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));
        return tsx_hip_sync(m);
    }
};

extern "C" int tsx_hip_load_host(tsx_hip_map *m, int fd, size_t chunk_bytes, uint64_t *entries_out) {
    if (entries_out) *entries_out = 0;
    if (!m || fd < 0) return TSX_HIP_EINVAL;
    if (m->p.lg != m->p.l) { g_last_error = "a shard of a multi-GPU table does not load a database"; return TSX_HIP_EINVAL; }
    tsx_hip_db_info d;
    uint64_t carry_sum = 0;
    TSX_TRY(db_read_header(m, fd, &d, &carry_sum));
    HIP_TRY(hipSetDevice(m->device));
    join_foreign(m, false);
    DbLoad ld(m, fd, d, carry_sum, chunk_bytes ? chunk_bytes : DB_CHUNK_DEFAULT);
    int rc = ld.begin();
    if (rc == TSX_HIP_OK) rc = ld.carry_section();
    if (rc == TSX_HIP_OK) rc = ld.chunks();
    if (rc == TSX_HIP_OK) rc = ld.end();
    if (entries_out) *entries_out = ld.entries;
    return rc;
}

// ---- table set operations (tsx_combine.h) ------------------------------------------------------------------------
static const size_t COMBINE_CHUNK_DEFAULT = (size_t)256 << 20;   // bytes of one staging chunk of (k-mer, count)

static int combine_fail(const char *why) { g_last_error = why; return TSX_HIP_EINVAL; }

// l, slot layout, segment bits and seed agree: a hashed key has the same home slot and the same slot words in both.
static bool combine_aligned(const tsx_hip_map *x, const tsx_hip_map *y) {
    return x->p.l == y->p.l && x->p.W == y->p.W && x->p.F == y->p.F && x->p.R == y->p.R && x->p.C == y->p.C &&
           x->p.S == y->p.S && x->seed == y->seed;
}

// The arguments and whether the tables can be combined at all.
static int combine_check(const tsx_hip_map *out, const tsx_hip_map *a, const tsx_hip_map *b, const tsx_hip_combine_rule *rule) {
    if (!a || !b || !rule) return combine_fail("combine: a, b and the rule are needed");
    if (rule->op < TSX_HIP_OP_INTERSECT || rule->op > TSX_HIP_OP_DIFF) return combine_fail("combine: unknown op");
    if (rule->count_mode < TSX_HIP_CNT_MIN || rule->count_mode > TSX_HIP_CNT_RIGHT) return combine_fail("combine: unknown count mode");
    if (std::max<uint64_t>(1, rule->a_lower) > rule->a_upper || std::max<uint64_t>(1, rule->b_lower) > rule->b_upper)
        return combine_fail("combine: lower > upper");
    if (out && (out == a || out == b)) return combine_fail("combine: out is one of the inputs");
    for (const tsx_hip_map *m : {a, b, out}) {
        if (!m) continue;
        if (m->p.lg != m->p.l) return combine_fail("combine: a shard of a multi-GPU table");
        if (m->device != a->device) return combine_fail("combine: the tables are on different devices");
        if (m->p.k != a->p.k) return combine_fail("combine: the tables differ in k");
        if (m->canon != a->canon) return combine_fail("combine: the tables differ in canonical mode");
        if (m->p.acgt_only != a->p.acgt_only || m->minq != a->minq) return combine_fail("combine: the tables differ in base rule");
    }
    if (out && out->used) return combine_fail("combine: out is not empty");
    return TSX_HIP_OK;
}

// Which sweep runs and where its survivors go.  TSX_HIP_COMBINE_PATH: 0 = by the tables (default), 1 = the general path,
// 2 = the aligned path; TSX_HIP_COMBINE_CHUNK_BYTES: the bytes of one staging chunk.  (Tests use the paths as each
// other's reference.)
struct CombinePath {
    bool aligned;          // A and B are joined slot against slot
    bool fused;            // ... and the survivors go into OUT by hashed key: no staging
    uint64_t chunk_slots;  // slots swept into one staging chunk
};
static int combine_path(const tsx_hip_map *out, const tsx_hip_map *a, const tsx_hip_map *b, CombinePath *cp) {
    int path = 0;
    if (const char *e = getenv("TSX_HIP_COMBINE_PATH")) path = atoi(e);
    const bool ab_aligned = combine_aligned(a, b);
    if (path < 0 || path > 2) return combine_fail("combine: TSX_HIP_COMBINE_PATH is 0, 1 or 2");
    if (path == 2 && !ab_aligned) return combine_fail("combine: the aligned path needs A and B of one l, slot layout, segment bits and seed");
    cp->aligned = path == 2 || (path == 0 && ab_aligned);
    cp->fused = cp->aligned && out && combine_aligned(a, out);
    size_t chunk_bytes = COMBINE_CHUNK_DEFAULT;
    if (const char *e = getenv("TSX_HIP_COMBINE_CHUNK_BYTES")) { const long long v = atoll(e); if (v > 0) chunk_bytes = (size_t)v; }
    const uint64_t max_slots = std::max(a->lay.slots, b->lay.slots);
    cp->chunk_slots = std::min<uint64_t>(max_slots, std::max<uint64_t>(64, (chunk_bytes / ((size_t)(a->p.wk + 1) * 8)) & ~(uint64_t)63));
    return TSX_HIP_OK;
}

// Staging of the paths that go through k-mers: two chunks, so that add_kmers_kernel inserts one (on OUT's stream)
// while the sweep fills the other (on the sweep stream sw).
struct CombineStage {
    DevBuf<uint64_t> d_kmers[2], d_counts[2];
    DevBuf<unsigned long long> d_n;   // entries staged per chunk
    PinBuf<unsigned long long> h_n;
    Event swept[2], inserted[2];
    bool waiting[2] = {false, false}, reuse[2] = {false, false};
    uint64_t chunk = 0;               // chunks swept so far: the next one goes into buffer chunk & 1

    int init(uint64_t chunk_slots, int WK) {
        if (d_n.alloc(2 * 8) != TSX_HIP_OK || h_n.alloc(2 * 8) != TSX_HIP_OK) return TSX_HIP_ENOMEM;
        for (int i = 0; i < 2; ++i) {
            if (d_kmers[i].alloc((size_t)chunk_slots * WK * 8) != TSX_HIP_OK || d_counts[i].alloc((size_t)chunk_slots * 8) != TSX_HIP_OK) {
                g_last_error = "combine: staging";
                return TSX_HIP_ENOMEM;
            }
            if (swept[i].create() != TSX_HIP_OK || inserted[i].create() != TSX_HIP_OK) return TSX_HIP_EHIP;
        }
        return TSX_HIP_OK;
    }
    // the chunk in buffer i has been swept: insert it into OUT
    int insert_chunk(int i, tsx_hip_map *out) {
        waiting[i] = false;
        HIP_TRY(hipEventSynchronize(swept[i].get()));
        const unsigned long long n = h_n.get()[i];
        if (n == 0) return TSX_HIP_OK;
        TSX_TRY(tsx_hip_add_kmers_device(out, d_kmers[i].get(), d_counts[i].get(), (size_t)n, nullptr));
        HIP_TRY(hipEventRecord(inserted[i].get(), out->stream.get()));
        reuse[i] = true;
        return TSX_HIP_OK;
    }
    // the next buffer, free for a sweep on sw: what it held is on its way into OUT, its counter is zeroed
    int next_buffer(hipStream_t sw, tsx_hip_map *out) {
        const int i = (int)(chunk & 1);
        if (waiting[i]) TSX_TRY(insert_chunk(i, out));
        if (reuse[i]) HIP_TRY(hipStreamWaitEvent(sw, inserted[i].get(), 0));
        HIP_TRY(hipMemsetAsync(d_n.get() + i, 0, 8, sw));
        return TSX_HIP_OK;
    }
    // that buffer's sweep is queued: its count comes back, and the chunk before it is inserted while it is swept
    int sweep_queued(hipStream_t sw, tsx_hip_map *out) {
        const int i = (int)(chunk & 1);
        HIP_TRY(hipMemcpyAsync(h_n.get() + i, d_n.get() + i, 8, hipMemcpyDeviceToHost, sw));
        HIP_TRY(hipEventRecord(swept[i].get(), sw));
        waiting[i] = true;
        ++chunk;
        return waiting[chunk & 1] ? insert_chunk((int)(chunk & 1), out) : TSX_HIP_OK;
    }
    // after the last sweep: the (at most two) chunks still waiting, the older one first
    int drain(tsx_hip_map *out) {
        for (int i = 0; i < 2; ++i)
            if (waiting[(chunk + i) & 1]) TSX_TRY(insert_chunk((int)((chunk + i) & 1), out));
        return TSX_HIP_OK;
    }
};

// The sweep's arguments for a side (0: src = A, 1: src = B); a_sec / b_sec: the table has carried counts.
static CombineArgs combine_args(const tsx_hip_combine_rule *rule, int side, bool a_sec, bool b_sec, int emit) {
    const uint64_t a_lo = std::max<uint64_t>(1, rule->a_lower), b_lo = std::max<uint64_t>(1, rule->b_lower);
    CombineArgs ca;
    ca.op = rule->op; ca.mode = rule->count_mode; ca.side = side; ca.emit = emit;
    ca.src_sec = side == 0 ? a_sec : b_sec; ca.oth_sec = side == 0 ? b_sec : a_sec;
    ca.s_lo = side == 0 ? a_lo : b_lo; ca.s_hi = side == 0 ? rule->a_upper : rule->b_upper;
    ca.o_lo = side == 0 ? b_lo : a_lo; ca.o_hi = side == 0 ? rule->b_upper : rule->a_upper;
    return ca;
}

// combine_sweep_kernel over slots [lo, hi) of src on stream sw; dk, dc, dn: the staging buffer and its counter (emit == 1).
static int combine_sweep_launch(const tsx_hip_map *a, bool aligned, const TableParams &src, const TableParams &oth,
                                const TableParams &po, const CombineArgs &ca, uint64_t lo, uint64_t hi, uint64_t *dk, uint64_t *dc,
                                unsigned long long *dn, unsigned long long *d_res, hipStream_t sw) {
    const int grid = (int)std::max<uint64_t>(1, std::min<uint64_t>((hi - lo + CB_TILE - 1) / CB_TILE, (uint64_t)a->cus * 8));
    if (aligned) {
        DISPATCH_WK(a, hipLaunchKernelGGL((combine_sweep_kernel<WKV, false, true>), dim3(grid), dim3(NT), 0, sw, src, oth, po, ca,
                                          lo, hi, dk, dc, (uint64_t)(hi - lo), dn, d_res));
    } else {
        DISPATCH_CANON(a, DISPATCH_WK(a, hipLaunchKernelGGL((combine_sweep_kernel<WKV, CANV, false>), dim3(grid), dim3(NT), 0, sw,
                                                            src, oth, po, ca, lo, hi, dk, dc, (uint64_t)(hi - lo), dn, d_res)));
    }
    if (hipGetLastError() != hipSuccess) { g_last_error = "combine_sweep_kernel launch"; return TSX_HIP_EHIP; }
    return TSX_HIP_OK;
}

// One side's sweep: the whole table at once, or (ca.emit == 1) chunk by chunk through the staging.
static int combine_sweep_side(const tsx_hip_map *a, const tsx_hip_map *src, const tsx_hip_map *oth, tsx_hip_map *out,
                              const CombinePath &cp, const CombineArgs &ca, CombineStage &sg, unsigned long long *d_res,
                              hipStream_t sw) {
    const uint64_t slots = src->lay.slots, span = ca.emit == 1 ? cp.chunk_slots : slots;
    const TableParams &po = out ? out->p : src->p;
    for (uint64_t lo = 0; lo < slots; lo += span) {
        const uint64_t hi = std::min(slots, lo + span);
        if (ca.emit != 1) {
            TSX_TRY(combine_sweep_launch(a, cp.aligned, src->p, oth->p, po, ca, lo, hi, nullptr, nullptr, nullptr, d_res, sw));
            continue;
        }
        const int i = (int)(sg.chunk & 1);
        TSX_TRY(sg.next_buffer(sw, out));
        TSX_TRY(combine_sweep_launch(a, cp.aligned, src->p, oth->p, po, ca, lo, hi, sg.d_kmers[i].get(), sg.d_counts[i].get(),
                                     sg.d_n.get() + i, d_res, sw));
        TSX_TRY(sg.sweep_queued(sw, out));
    }
    return TSX_HIP_OK;
}

extern "C" int tsx_hip_combine(tsx_hip_map *out, tsx_hip_map *a, tsx_hip_map *b, const tsx_hip_combine_rule *rule,
                               tsx_hip_combine_stats *stats_out) {
    if (stats_out) memset(stats_out, 0, sizeof *stats_out);
    TSX_TRY(combine_check(out, a, b, rule));
    CombinePath cp;
    TSX_TRY(combine_path(out, a, b, &cp));
    HIP_TRY(hipSetDevice(a->device));
    // behind everything queued on the three maps; lazily cleared tables are zeroed before anyone reads them
    for (tsx_hip_map *m : {a, b, out}) {
        if (!m) continue;
        join_foreign(m, true);
        TSX_TRY(ensure_zeroed(m, m->stream.get()));
        HIP_TRY(hipStreamSynchronize(m->stream.get()));
    }
    unsigned long long a_carry = 0, b_carry = 0;
    HIP_TRY(hipMemcpy(&a_carry, a->p.stats + ST_CARRY, 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&b_carry, b->p.stats + ST_CARRY, 8, hipMemcpyDeviceToHost));

    hipStream_t sw = a->stream.get();   // the sweeps; the inserts of staged chunks run on OUT's stream
    CombineStage sg;
    DevBuf<unsigned long long> res;
    SyncAtExit wait_sw(sw), wait_out(out ? out->stream.get() : sw);   // nothing queued may outlive the staging
    if (res.alloc(CB_N * 8) != TSX_HIP_OK) return TSX_HIP_ENOMEM;
    HIP_TRY(hipMemsetAsync(res.get(), 0, CB_N * 8, sw));
    const bool staging = out && !cp.fused;
    if (staging) TSX_TRY(sg.init(cp.chunk_slots, a->p.wk));
    for (int side = 0; side < 2; ++side) {
        // B's sweep writes only for UNION; for the other ops it counts b_in_range
        const bool writes = out && (side == 0 || rule->op == TSX_HIP_OP_UNION);
        if (side == 1 && !writes && !stats_out) break;
        const CombineArgs ca = combine_args(rule, side, a_carry != 0, b_carry != 0, !writes ? 0 : cp.fused ? 2 : 1);
        if (ca.emit == 2) out->used = true;   // (the sweep itself inserts; OUT's stream is idle, see above)
        TSX_TRY(combine_sweep_side(a, side == 0 ? a : b, side == 0 ? b : a, out, cp, ca, sg, res.get(), sw));
    }
    if (staging) TSX_TRY(sg.drain(out));
    unsigned long long h_res[CB_N] = {0};
    HIP_TRY(hipMemcpyAsync(h_res, res.get(), CB_N * 8, hipMemcpyDeviceToHost, sw));
    HIP_TRY(hipStreamSynchronize(sw));
    if (stats_out) {
        stats_out->a_in_range = h_res[CB_A_IN]; stats_out->b_in_range = h_res[CB_B_IN]; stats_out->both = h_res[CB_BOTH];
        stats_out->a_sum_both = h_res[CB_A_SUM]; stats_out->b_sum_both = h_res[CB_B_SUM];
        stats_out->out_entries = h_res[CB_OUT_N]; stats_out->out_count_sum = h_res[CB_OUT_SUM];
    }
    return out ? tsx_hip_sync(out) : TSX_HIP_OK;
}

// ---- joint spectrum of two tables (tsx_joint.h) ------------------------------------------------------------------
static const size_t JOINT_MAX_CELLS = (size_t)1 << 24;

static int joint_check(const tsx_hip_map *a, const tsx_hip_map *b, size_t na, size_t nb) {
    if (!a || !b) return combine_fail("joint histogram: a and b are needed");
    if (a->p.lg != a->p.l || b->p.lg != b->p.l) return combine_fail("joint histogram: a shard of a multi-GPU table");
    if (b->device != a->device) return combine_fail("joint histogram: the tables are on different devices");
    if (b->p.k != a->p.k) return combine_fail("joint histogram: the tables differ in k");
    if (b->canon != a->canon) return combine_fail("joint histogram: the tables differ in canonical mode");
    if (b->p.acgt_only != a->p.acgt_only || b->minq != a->minq) return combine_fail("joint histogram: the tables differ in base rule");
    if (na < 2 || nb < 2) return combine_fail("joint histogram: fewer than 2 bins");
    if (na > JOINT_MAX_CELLS || nb > JOINT_MAX_CELLS || na * nb > JOINT_MAX_CELLS) return combine_fail("joint histogram: more than 2^24 cells");
    return TSX_HIP_OK;
}

// joint_histogram_kernel over every slot of src on stream st.
static int joint_launch(const tsx_hip_map *a, bool aligned, const tsx_hip_map *src, const tsx_hip_map *oth, const JointArgs &ja,
                        size_t na, size_t nb, unsigned long long *d_matrix, hipStream_t st) {
    const uint64_t slots = src->lay.slots, tiles = (slots + JH_TILE - 1) / JH_TILE;
    uint64_t grid = std::max<uint64_t>(1, std::min<uint64_t>(tiles, (uint64_t)a->cus * 8));
    // A workgroup's corner is u32: bound the slots one workgroup sweeps below 2^31.
    auto per_wg = [&](uint64_t g) { return (tiles + g - 1) / g * JH_TILE; };
    while (per_wg(grid) >= (1ULL << 31) && grid < (1ULL << 30)) grid *= 2;
    if (per_wg(grid) >= (1ULL << 31)) return combine_fail("joint histogram: the table is too large");
    if (aligned) {
        DISPATCH_WK(a, hipLaunchKernelGGL((joint_histogram_kernel<WKV, false, true>), dim3((unsigned)grid), dim3(NT), 0, st, src->p,
                                          oth->p, ja, (uint64_t)0, slots, (uint32_t)na, (uint32_t)nb, d_matrix));
    } else {
        DISPATCH_CANON(a, DISPATCH_WK(a, hipLaunchKernelGGL((joint_histogram_kernel<WKV, CANV, false>), dim3((unsigned)grid), dim3(NT),
                                                            0, st, src->p, oth->p, ja, (uint64_t)0, slots, (uint32_t)na,
                                                            (uint32_t)nb, d_matrix)));
    }
    if (hipGetLastError() != hipSuccess) { g_last_error = "joint_histogram_kernel launch"; return TSX_HIP_EHIP; }
    return TSX_HIP_OK;
}

extern "C" int tsx_hip_joint_histogram_device(tsx_hip_map *a, tsx_hip_map *b, size_t na, size_t nb, void *dev_matrix, void *stream) {
    TSX_TRY(joint_check(a, b, na, nb));
    if (!dev_matrix) return combine_fail("joint histogram: no matrix");
    CombinePath cp;
    TSX_TRY(combine_path(nullptr, a, b, &cp));
    HIP_TRY(hipSetDevice(a->device));
    // behind everything queued on the two maps; lazily cleared tables are zeroed before anyone reads them
    for (tsx_hip_map *m : {a, b}) {
        join_foreign(m, true);
        TSX_TRY(ensure_zeroed(m, m->stream.get()));
        HIP_TRY(hipStreamSynchronize(m->stream.get()));
    }
    unsigned long long a_carry = 0, b_carry = 0;
    HIP_TRY(hipMemcpy(&a_carry, a->p.stats + ST_CARRY, 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&b_carry, b->p.stats + ST_CARRY, 8, hipMemcpyDeviceToHost));
    hipStream_t st = pick_stream(a, stream);   // (both maps' streams are idle: nothing for st to wait for)
    unsigned long long *d_matrix = (unsigned long long *)dev_matrix;
    HIP_TRY(hipMemsetAsync(d_matrix, 0, na * nb * sizeof(unsigned long long), st));
    for (int side = 0; side < (a == b ? 1 : 2); ++side) {
        JointArgs ja;
        ja.side = side;
        ja.src_sec = (side == 0 ? a_carry : b_carry) != 0;
        ja.oth_sec = (side == 0 ? b_carry : a_carry) != 0;
        TSX_TRY(joint_launch(a, cp.aligned, side == 0 ? a : b, side == 0 ? b : a, ja, na, nb, d_matrix, st));
    }
    // what B's own stream does next goes behind the sweeps (A: pick_stream remembers a caller's stream)
    if (st != b->stream.get() && b->join_ev.get()) {
        HIP_TRY(hipEventRecord(b->join_ev.get(), st));
        HIP_TRY(hipStreamWaitEvent(b->stream.get(), b->join_ev.get(), 0));
    }
    return TSX_HIP_OK;
}

extern "C" int tsx_hip_joint_histogram_host(tsx_hip_map *a, tsx_hip_map *b, uint64_t *matrix_out, size_t na, size_t nb) {
    TSX_TRY(joint_check(a, b, na, nb));
    if (!matrix_out) return combine_fail("joint histogram: no matrix");
    HIP_TRY(hipSetDevice(a->device));
    DevBuf<uint64_t> d;
    TSX_TRY(d.alloc(na * nb * sizeof(uint64_t)));
    SyncAtExit wait_a(a->stream.get());   // nothing queued may outlive the matrix
    TSX_TRY(tsx_hip_joint_histogram_device(a, b, na, nb, d.get(), nullptr));
    HIP_TRY(hipMemcpyAsync(matrix_out, d.get(), na * nb * sizeof(uint64_t), hipMemcpyDeviceToHost, a->stream.get()));
    HIP_TRY(hipStreamSynchronize(a->stream.get()));
    return TSX_HIP_OK;
}

// ---- heterozygous pairs of one table (tsx_het.h; DESIGN.md §3 "Heterozygous pairs") ------------------------------
static int het_check(const tsx_hip_map *m, const tsx_hip_het_rule *rule) {
    if (!m || !rule) return combine_fail("het pairs: a map and a rule are needed");
    if (!(m->p.k & 1)) return combine_fail("het pairs: even k (no middle base)");
    if (m->p.lg != m->p.l) return combine_fail("het pairs: a map created with shard_bits > 0");
    if (rule->lower > rule->upper) return combine_fail("het pairs: lower > upper");
    if (rule->mode != TSX_HIP_HET_UNIQUE && rule->mode != TSX_HIP_HET_ALL) return combine_fail("het pairs: unknown mode");
    if (rule->reserved != 0) return combine_fail("het pairs: reserved must be 0");
    return TSX_HIP_OK;
}
static int het_check_bins(size_t n_minor, size_t n_major) {
    if (n_minor < 2 || n_major < 2) return combine_fail("het histogram: fewer than 2 bins");
    if (n_minor > JOINT_MAX_CELLS || n_major > JOINT_MAX_CELLS || n_minor * n_major > JOINT_MAX_CELLS)
        return combine_fail("het histogram: more than 2^24 cells");
    return TSX_HIP_OK;
}

// The kernel's view of the rule: the range, the mode, the middle base and H_d = A * (d << 2p) for d = 1..3.
static HetArgs het_args(const tsx_hip_map *m, const tsx_hip_het_rule *rule, bool sec) {
    HetArgs ha;
    memset(&ha, 0, sizeof ha);
    ha.lower = std::max<uint64_t>(rule->lower, 1);
    ha.upper = rule->upper;
    ha.mode = rule->mode;
    ha.sec = sec ? 1 : 0;
    const int bit = 2 * ((m->p.k - 1) / 2);
    ha.mid_limb = bit >> 6;
    ha.mid_shift = bit & 63;
    for (uint64_t d = 1; d <= 3; ++d) {
        uint64_t x[4] = {0, 0, 0, 0};
        x[ha.mid_limb] = d << ha.mid_shift;
        apply_rows(m, m->rows, x, ha.hd[d - 1]);
    }
    return ha;
}

// Everything queued on the map has finished, a lazily cleared table is zeroed; *sec = the table ever carried.
static int het_settle(tsx_hip_map *m, bool *sec) {
    join_foreign(m, true);
    TSX_TRY(ensure_zeroed(m, m->stream.get()));
    HIP_TRY(hipStreamSynchronize(m->stream.get()));
    unsigned long long carry = 0;
    HIP_TRY(hipMemcpy(&carry, m->p.stats + ST_CARRY, 8, hipMemcpyDeviceToHost));
    *sec = carry != 0;
    return TSX_HIP_OK;
}

// het_sweep_kernel over slots [lo, hi) on stream st: the matrix and stats form (d_pairs == nullptr && !list) or the list form.
static int het_launch(const tsx_hip_map *m, const HetArgs &ha, bool list, uint64_t lo, uint64_t hi, size_t n_minor, size_t n_major,
                      unsigned long long *d_matrix, unsigned long long *d_stats, uint64_t *d_pairs, uint64_t cap,
                      unsigned long long *d_n, hipStream_t st) {
    if (hi == lo) return TSX_HIP_OK;
    const uint64_t tiles = (hi - lo + HET_TILE - 1) / HET_TILE;
    uint64_t grid = std::max<uint64_t>(1, std::min<uint64_t>(tiles, (uint64_t)m->cus * 8));
    // A workgroup's corner and a lane's sums are u32: bound the slots one workgroup sweeps below 2^31.
    auto per_wg = [&](uint64_t g) { return (tiles + g - 1) / g * HET_TILE; };
    while (per_wg(grid) >= (1ULL << 31) && grid < (1ULL << 30)) grid *= 2;
    if (per_wg(grid) >= (1ULL << 31)) return combine_fail("het pairs: the table is too large");
    if (list) {
        DISPATCH_CANON(m, DISPATCH_WK(m, hipLaunchKernelGGL((het_sweep_kernel<WKV, CANV, true>), dim3((unsigned)grid), dim3(NT), 0, st,
                                                            m->p, ha, lo, hi, 0u, 0u, (unsigned long long *)nullptr,
                                                            (unsigned long long *)nullptr, d_pairs, cap, d_n)));
    } else {
        DISPATCH_CANON(m, DISPATCH_WK(m, hipLaunchKernelGGL((het_sweep_kernel<WKV, CANV, false>), dim3((unsigned)grid), dim3(NT), 0, st,
                                                            m->p, ha, lo, hi, (uint32_t)n_minor, (uint32_t)n_major, d_matrix, d_stats,
                                                            (uint64_t *)nullptr, (uint64_t)0, (unsigned long long *)nullptr)));
    }
    if (hipGetLastError() != hipSuccess) { g_last_error = "het_sweep_kernel launch"; return TSX_HIP_EHIP; }
    return TSX_HIP_OK;
}

extern "C" int tsx_hip_het_histogram_device(tsx_hip_map *m, const tsx_hip_het_rule *rule, size_t n_minor, size_t n_major,
                                            void *dev_matrix, void *dev_stats, void *stream) {
    TSX_TRY(het_check(m, rule));
    TSX_TRY(het_check_bins(n_minor, n_major));
    if (!dev_matrix || !dev_stats) return combine_fail("het histogram: no matrix or no stats");
    HIP_TRY(hipSetDevice(m->device));
    bool sec = false;
    TSX_TRY(het_settle(m, &sec));
    hipStream_t st = pick_stream(m, stream);   // (the map's stream is idle: nothing for st to wait for)
    HIP_TRY(hipMemsetAsync(dev_matrix, 0, n_minor * n_major * sizeof(unsigned long long), st));
    HIP_TRY(hipMemsetAsync(dev_stats, 0, sizeof(tsx_hip_het_stats), st));
    static_assert(sizeof(tsx_hip_het_stats) == HS_N * 8, "tsx_hip_het_stats is the kernel's HS_N totals");
    return het_launch(m, het_args(m, rule, sec), false, 0, m->lay.slots, n_minor, n_major, (unsigned long long *)dev_matrix,
                      (unsigned long long *)dev_stats, nullptr, 0, nullptr, st);
}

extern "C" int tsx_hip_het_histogram_host(tsx_hip_map *m, const tsx_hip_het_rule *rule, uint64_t *matrix_out, size_t n_minor,
                                          size_t n_major, tsx_hip_het_stats *stats_out) {
    TSX_TRY(het_check(m, rule));
    TSX_TRY(het_check_bins(n_minor, n_major));
    if (!matrix_out) return combine_fail("het histogram: no matrix");
    HIP_TRY(hipSetDevice(m->device));
    const size_t cells = n_minor * n_major;
    DevBuf<uint64_t> d;
    TSX_TRY(d.alloc((cells + HS_N) * sizeof(uint64_t)));
    SyncAtExit wait(m->stream.get());   // nothing queued may outlive the matrix
    TSX_TRY(tsx_hip_het_histogram_device(m, rule, n_minor, n_major, d.get(), d.get() + cells, nullptr));
    tsx_hip_het_stats s;
    HIP_TRY(hipMemcpyAsync(matrix_out, d.get(), cells * sizeof(uint64_t), hipMemcpyDeviceToHost, m->stream.get()));
    HIP_TRY(hipMemcpyAsync(&s, d.get() + cells, sizeof s, hipMemcpyDeviceToHost, m->stream.get()));
    HIP_TRY(hipStreamSynchronize(m->stream.get()));
    if (stats_out) *stats_out = s;
    return TSX_HIP_OK;
}

extern "C" int tsx_hip_het_pairs_device(tsx_hip_map *m, const tsx_hip_het_rule *rule, uint64_t slot_lo, uint64_t slot_hi,
                                        void *dev_pairs, size_t cap, void *dev_n, void *stream) {
    TSX_TRY(het_check(m, rule));
    if (!dev_n || (!dev_pairs && cap)) return combine_fail("het pairs: no output");
    if (slot_lo > slot_hi || slot_hi > m->lay.slots) return combine_fail("het pairs: slot range");
    HIP_TRY(hipSetDevice(m->device));
    bool sec = false;
    TSX_TRY(het_settle(m, &sec));
    hipStream_t st = pick_stream(m, stream);
    HIP_TRY(hipMemsetAsync(dev_n, 0, sizeof(unsigned long long), st));
    TSX_TRY(het_launch(m, het_args(m, rule, sec), true, slot_lo, slot_hi, 0, 0, nullptr, nullptr, (uint64_t *)dev_pairs, (uint64_t)cap,
                       (unsigned long long *)dev_n, st));
    unsigned long long n = 0;
    HIP_TRY(hipMemcpyAsync(&n, dev_n, sizeof n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return n > cap ? TSX_HIP_ERANGE : TSX_HIP_OK;
}

// The pair list as text.  A chunk of S slots owns at most S pairs (unique) or 3 S (all): its records and its text always fit.
extern "C" int tsx_hip_write_het_pairs_host(tsx_hip_map *m, const tsx_hip_het_rule *rule, int fd, size_t chunk_bytes,
                                            uint64_t *pairs_out, uint64_t *bytes_out) {
    if (pairs_out) *pairs_out = 0;
    if (bytes_out) *bytes_out = 0;
    TSX_TRY(het_check(m, rule));
    if (fd < 0) return combine_fail("het pairs: no output");
    const int k = m->p.k, wk = m->p.wk;
    const size_t line = 2 * ((size_t)k + 21) + 2, per_slot = rule->mode == TSX_HIP_HET_ALL ? 3 : 1;   // 2 x (bases, TAB, 20 digits), newline
    const size_t rec_words = 2 * (size_t)wk + 2;
    if (!chunk_bytes) chunk_bytes = WRITE_CHUNK_DEFAULT;
    const uint64_t slots = m->lay.slots, per = std::min<uint64_t>(chunk_bytes / (line * per_slot), slots);
    if (per < std::min<uint64_t>(64, slots)) return combine_fail("het pairs: chunk_bytes holds fewer than 64 slots");
    const uint64_t cap = per * per_slot;
    HIP_TRY(hipSetDevice(m->device));
    bool sec = false;
    TSX_TRY(het_settle(m, &sec));
    const HetArgs ha = het_args(m, rule, sec);
    hipStream_t st = m->stream.get();
    ChunkAhead ahead(st, slots, per);
    TSX_TRY(ahead.init((size_t)cap * rec_words * 8, 2));
    std::vector<uint8_t> text;
    uint64_t pairs = 0, bytes = 0;
    const int rc = ahead.run(
        [&](uint64_t lo, uint64_t hi, uint8_t *d_rec, unsigned long long *d_n, unsigned long long *h_n) -> int {
            HIP_TRY(hipMemsetAsync(d_n, 0, 2 * 8, st));
            TSX_TRY(het_launch(m, ha, true, lo, hi, 0, 0, nullptr, nullptr, (uint64_t *)d_rec, cap, d_n, st));
            HIP_TRY(hipMemcpyAsync(h_n, d_n, 2 * 8, hipMemcpyDeviceToHost, st));
            return TSX_HIP_OK;
        },
        [&](uint64_t, uint64_t, const unsigned long long *n, ChunkAhead::Range *r) -> int {
            if (n[0] > cap) return TSX_HIP_ERANGE;   // cannot happen: a slot owns at most per_slot pairs
            r[0].n = (size_t)n[0] * rec_words * 8;
            return TSX_HIP_OK;
        },
        [&](uint64_t, uint64_t, const unsigned long long *n, const uint8_t *h_rec, const ChunkAhead::Range *) -> int {
            text.resize((size_t)n[0] * line + 8);   // (+ the NUL that decode and snprintf put behind what they write)
            size_t at = 0;
            for (uint64_t i = 0; i < n[0]; ++i) {
                const uint64_t *rec = (const uint64_t *)h_rec + i * rec_words;
                for (int side = 0; side < 2; ++side) {
                    tsx_hip_decode(rec + side * wk, k, (char *)text.data() + at);
                    at += (size_t)k;
                    at += (size_t)snprintf((char *)text.data() + at, 24, "\t%llu%c", (unsigned long long)rec[2 * wk + side], side ? '\n' : '\t');
                }
            }
            TSX_TRY(write_all(fd, text.data(), at));
            bytes += at; pairs += n[0];
            return TSX_HIP_OK;
        });
    if (pairs_out) *pairs_out = pairs;
    if (bytes_out) *bytes_out = bytes;
    return rc;
}

// ---- unitigs: the compacted de Bruijn graph of one table (tsx_unitig.h; DESIGN.md §3 "Unitigs") --------------------------
static int unitig_check(const tsx_hip_map *m, const tsx_hip_unitig_rule *rule) {
    if (!m || !rule) return combine_fail("unitigs: a map and a rule are needed");
    if (m->p.lg != m->p.l) return combine_fail("unitigs: a map created with shard_bits > 0");
    if (rule->lower > rule->upper) return combine_fail("unitigs: lower > upper");
    if (rule->flags != 0 || rule->reserved != 0) return combine_fail("unitigs: flags and reserved must be 0");
    if (m->canon && !(m->p.k & 1)) return combine_fail("unitigs: even k on a canonical table");
    return TSX_HIP_OK;
}
static_assert(sizeof(tsx_hip_unitig_totals) == UT_PUBLIC * 8, "tsx_hip_unitig_totals is the kernels' first UT_PUBLIC totals");
static_assert(sizeof(tsx_hip_unitig) == sizeof(UnitigRec), "tsx_hip_unitig is the kernels' record");

// What the steps of the last unitig call of this thread took, in ms (host clock; every step waits for its totals): the
// degree sweep, the walk of the starts, the spelling walk, the cycle pass (tsx_hip_unitig_last_timing).
static thread_local double g_unitig_ms[4] = {0, 0, 0, 0};

// One call's scratch and its three steps, all on st: degrees() = stage 1, walks() = stages 2 and 4, spell() = stage 3.
// Each waits for its totals (h).  Extra device memory: one byte and one bit per slot, 8 bytes per record asked for.
struct UnitigRun {
    tsx_hip_map *m;
    hipStream_t st;
    UnitigArgs ua;
    uint64_t slots = 0, grid = 1, rec_room = 0;
    DevBuf<uint8_t> side;
    DevBuf<uint32_t> covered;
    DevBuf<unsigned long long> tot;
    DevBuf<uint64_t> start;
    unsigned long long h[UT_N];
    double t0 = 0;   // host clock at the start of the step under way: every step ends waiting for its totals

    static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
    void timed(int stage) { const double t = now_ms(); g_unitig_ms[stage] += t - t0; t0 = t; }

    int totals() {
        HIP_TRY(hipMemcpyAsync(h, tot.get(), sizeof h, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (h[UT_ERROR]) { g_last_error = "unitigs: the table is not consistent"; return TSX_HIP_EHIP; }
        return TSX_HIP_OK;
    }
    void publish(tsx_hip_unitig_totals *out) const { if (out) memcpy(out, h, sizeof *out); }

    int degrees(const tsx_hip_unitig_rule *rule, bool sec) {
        memset(&ua, 0, sizeof ua);
        memset(h, 0, sizeof h);
        for (double &v : g_unitig_ms) v = 0;
        ua.lower = std::max<uint64_t>(rule->lower, 1);
        ua.upper = rule->upper;
        ua.sec = sec ? 1 : 0;
        ua.top_shift = (2 * (m->p.k - 1)) & 63;
        for (uint64_t c = 1; c <= 3; ++c) {
            uint64_t x[4] = {0, 0, 0, 0};
            x[0] = c;
            apply_rows(m, m->rows, x, ua.lo[c]);
            x[0] = 0;
            x[m->p.wk - 1] = c << ua.top_shift;
            apply_rows(m, m->rows, x, ua.hi[c]);
        }
        slots = m->lay.slots;
        const uint64_t tiles = (slots + UNITIG_TILE - 1) / UNITIG_TILE;
        grid = std::max<uint64_t>(1, std::min<uint64_t>(tiles, (uint64_t)m->cus * 8));
        auto per_wg = [&](uint64_t g) { return (tiles + g - 1) / g * UNITIG_TILE; };   // the lanes' sums are u32
        while (per_wg(grid) >= (1ULL << 31) && grid < (1ULL << 30)) grid *= 2;
        if (per_wg(grid) >= (1ULL << 31)) return combine_fail("unitigs: the table is too large");
        TSX_TRY(side.alloc((size_t)slots));
        TSX_TRY(covered.alloc((size_t)((slots + 31) / 32) * 4));
        TSX_TRY(tot.alloc(UT_N * 8));
        HIP_TRY(hipMemsetAsync(covered.get(), 0, covered.cap(), st));
        HIP_TRY(hipMemsetAsync(tot.get(), 0, UT_N * 8, st));
        HIP_TRY(hipStreamSynchronize(st));
        t0 = now_ms();
        DISPATCH_CANON(m, DISPATCH_WK(m, hipLaunchKernelGGL((unitig_degree_kernel<WKV, CANV>), dim3((unsigned)grid), dim3(NT), 0, st, m->p,
                                                            ua, slots, side.get(), tot.get())));
        if (hipGetLastError() != hipSuccess) { g_last_error = "unitig_degree_kernel launch"; return TSX_HIP_EHIP; }
        TSX_TRY(totals());
        timed(0);
        ua.bound = h[UT_NODES] + 1;
        return TSX_HIP_OK;
    }

    // d_rec: room for rec_cap records (null: totals only).  At most min(rec_cap, nodes) are written.
    int walks(UnitigRec *d_rec, uint64_t rec_cap) {
        rec_room = d_rec ? std::min<uint64_t>(rec_cap, h[UT_NODES]) : 0;
        TSX_TRY(start.alloc((size_t)std::max<uint64_t>(rec_room, 1) * 8));
        t0 = now_ms();
        DISPATCH_CANON(m, DISPATCH_WK(m, hipLaunchKernelGGL((unitig_walk_kernel<WKV, CANV>), dim3((unsigned)grid), dim3(NT), 0, st, m->p, ua,
                                                            slots, side.get(), covered.get(), tot.get(), d_rec, start.get(), rec_room)));
        if (hipGetLastError() != hipSuccess) { g_last_error = "unitig_walk_kernel launch"; return TSX_HIP_EHIP; }
        TSX_TRY(totals());
        timed(1);
        DISPATCH_CANON(m, DISPATCH_WK(m, hipLaunchKernelGGL((unitig_cycle_kernel<WKV, CANV>), dim3((unsigned)grid), dim3(NT), 0, st, m->p, ua,
                                                            slots, side.get(), covered.get(), tot.get(), d_rec, start.get(), rec_room)));
        if (hipGetLastError() != hipSuccess) { g_last_error = "unitig_cycle_kernel launch"; return TSX_HIP_EHIP; }
        TSX_TRY(totals());
        timed(3);
        return TSX_HIP_OK;
    }

    // What walks() left is undone -- the covered bits and the four totals the walks add to -- so that it can run again.
    int forget_walks() {
        static_assert(UT_UNITIGS == 1 && UT_CIRCULAR == 2 && UT_BASES == 3 && UT_LONGEST == 4, "the walks' totals are words 1..4");
        HIP_TRY(hipMemsetAsync(covered.get(), 0, covered.cap(), st));
        HIP_TRY(hipMemsetAsync(tot.get() + UT_UNITIGS, 0, 4 * 8, st));
        return TSX_HIP_OK;
    }

    // The records are all there (unitigs <= rec_room) and seq_cap >= bases: the caller has checked.
    int spell(const UnitigRec *d_rec, uint8_t *d_seq, uint64_t seq_cap) {
        const uint64_t n = h[UT_UNITIGS];
        if (n > rec_room) { g_last_error = "unitigs: the table is not consistent"; return TSX_HIP_EHIP; }
        if (n == 0) return TSX_HIP_OK;
        const int g = grid_for(m, n, 8);
        t0 = now_ms();
        DISPATCH_CANON(m, DISPATCH_WK(m, hipLaunchKernelGGL((unitig_spell_kernel<WKV, CANV>), dim3(g), dim3(NT), 0, st, m->p, ua, side.get(),
                                                            d_rec, start.get(), n, seq_cap, d_seq, tot.get())));
        if (hipGetLastError() != hipSuccess) { g_last_error = "unitig_spell_kernel launch"; return TSX_HIP_EHIP; }
        TSX_TRY(totals());
        timed(2);
        return TSX_HIP_OK;
    }
};

// The map is settled and the run has its stream; a caller's stream is waited for before the scratch goes away.
static int unitig_begin(tsx_hip_map *m, const tsx_hip_unitig_rule *rule, void *stream, UnitigRun &run) {
    HIP_TRY(hipSetDevice(m->device));
    bool sec = false;
    TSX_TRY(het_settle(m, &sec));
    run.m = m;
    run.st = pick_stream(m, stream);
    return run.degrees(rule, sec);
}

extern "C" int tsx_hip_unitig_last_timing(double *ms_out) {
    if (!ms_out) return TSX_HIP_EINVAL;
    for (int i = 0; i < 4; ++i) ms_out[i] = g_unitig_ms[i];
    return TSX_HIP_OK;
}

extern "C" int tsx_hip_unitig_stats(tsx_hip_map *m, const tsx_hip_unitig_rule *rule, tsx_hip_unitig_totals *totals) {
    TSX_TRY(unitig_check(m, rule));
    if (!totals) return combine_fail("unitigs: no totals");
    UnitigRun run;
    SyncAtExit wait(m->stream.get());
    TSX_TRY(unitig_begin(m, rule, nullptr, run));
    TSX_TRY(run.walks(nullptr, 0));
    run.publish(totals);
    return TSX_HIP_OK;
}

extern "C" int tsx_hip_unitigs_device(tsx_hip_map *m, const tsx_hip_unitig_rule *rule, void *dev_seq, size_t seq_cap, void *dev_records,
                                      size_t record_cap, size_t *n_unitigs, size_t *seq_bytes, tsx_hip_unitig_totals *totals,
                                      void *stream) {
    TSX_TRY(unitig_check(m, rule));
    if (!n_unitigs || !seq_bytes || (!dev_seq && seq_cap) || (!dev_records && record_cap)) return combine_fail("unitigs: no output");
    *n_unitigs = *seq_bytes = 0;
    UnitigRun run;
    SyncAtExit wait(stream ? (hipStream_t)stream : m->stream.get());
    TSX_TRY(unitig_begin(m, rule, stream, run));
    TSX_TRY(run.walks(record_cap ? (UnitigRec *)dev_records : nullptr, record_cap));
    *n_unitigs = (size_t)run.h[UT_UNITIGS];
    *seq_bytes = (size_t)run.h[UT_BASES];
    run.publish(totals);
    if (run.h[UT_UNITIGS] > record_cap || run.h[UT_BASES] > seq_cap) return TSX_HIP_ERANGE;
    return run.spell((const UnitigRec *)dev_records, (uint8_t *)dev_seq, seq_cap);
}

// Record room (40 + 8 bytes a record) above which the walks run once for the number of unitigs before they run for the
// records: below it the room is simply min(record_cap, nodes).  TSX_HIP_UNITIG_SIZING_BYTES: tests take the sizing walk
// on small tables.
static uint64_t unitig_sizing_bytes() {
    if (const char *e = getenv("TSX_HIP_UNITIG_SIZING_BYTES")) return strtoull(e, nullptr, 10);
    return (uint64_t)256 << 20;
}

// Stages 1, 2 and 4 with records, then the sequences in a buffer of exactly their size.  The record room is
// min(record_cap, nodes); when that is large the walks first run without records and the room is the unitigs (one walk
// more, 48 bytes a unitig instead of 48 bytes a node).  ERANGE (sizes reported, nothing spelled) when a cap is too small.
static int unitig_make(tsx_hip_map *m, const tsx_hip_unitig_rule *rule, uint64_t seq_cap, uint64_t record_cap, UnitigRun &run,
                       DevBuf<UnitigRec> &d_rec, DevBuf<uint8_t> &d_seq) {
    TSX_TRY(unitig_begin(m, rule, nullptr, run));
    uint64_t room = std::min<uint64_t>(record_cap, run.h[UT_NODES]);
    if (room > unitig_sizing_bytes() / (sizeof(UnitigRec) + 8)) {
        TSX_TRY(run.walks(nullptr, 0));
        if (run.h[UT_UNITIGS] > record_cap || run.h[UT_BASES] > seq_cap) return TSX_HIP_ERANGE;
        room = run.h[UT_UNITIGS];
        TSX_TRY(run.forget_walks());
    }
    TSX_TRY(d_rec.alloc((size_t)std::max<uint64_t>(room, 1) * sizeof(UnitigRec)));
    TSX_TRY(run.walks(room ? d_rec.get() : nullptr, room));
    if (run.h[UT_UNITIGS] > record_cap || run.h[UT_BASES] > seq_cap) return TSX_HIP_ERANGE;
    TSX_TRY(d_seq.alloc((size_t)std::max<uint64_t>(run.h[UT_BASES], 1)));
    return run.spell(d_rec.get(), d_seq.get(), run.h[UT_BASES]);
}

extern "C" int tsx_hip_unitigs_host(tsx_hip_map *m, const tsx_hip_unitig_rule *rule, void *seq_out, size_t seq_cap,
                                    tsx_hip_unitig *records_out, size_t record_cap, size_t *n_unitigs, size_t *seq_bytes,
                                    tsx_hip_unitig_totals *totals) {
    TSX_TRY(unitig_check(m, rule));
    if (!n_unitigs || !seq_bytes || (!seq_out && seq_cap) || (!records_out && record_cap)) return combine_fail("unitigs: no output");
    *n_unitigs = *seq_bytes = 0;
    UnitigRun run;
    DevBuf<UnitigRec> d_rec;
    DevBuf<uint8_t> d_seq;
    SyncAtExit wait(m->stream.get());
    const int rc = unitig_make(m, rule, seq_cap, record_cap, run, d_rec, d_seq);
    if (rc != TSX_HIP_OK && rc != TSX_HIP_ERANGE) return rc;
    *n_unitigs = (size_t)run.h[UT_UNITIGS];
    *seq_bytes = (size_t)run.h[UT_BASES];
    run.publish(totals);
    if (rc != TSX_HIP_OK) return rc;
    hipStream_t st = m->stream.get();
    if (*n_unitigs) HIP_TRY(hipMemcpyAsync(records_out, d_rec.get(), *n_unitigs * sizeof(UnitigRec), hipMemcpyDeviceToHost, st));
    if (*seq_bytes) HIP_TRY(hipMemcpyAsync(seq_out, d_seq.get(), *seq_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return TSX_HIP_OK;
}

// FASTA behind the device: the records come over whole and are put in the order of their offsets -- they tile the
// sequence buffer -- then the sequences follow in pieces of whole records through two pinned buffers, piece i + 1 on its
// way while piece i is formatted and written.
extern "C" int tsx_hip_write_unitigs_host(tsx_hip_map *m, const tsx_hip_unitig_rule *rule, int fd, tsx_hip_unitig_totals *totals) {
    TSX_TRY(unitig_check(m, rule));
    if (fd < 0) return combine_fail("unitigs: no output");
    UnitigRun run;
    DevBuf<UnitigRec> d_rec;
    DevBuf<uint8_t> d_seq;
    PinBuf<uint8_t> pin[2];
    Event ready[2];
    SyncAtExit wait(m->stream.get());
    TSX_TRY(unitig_make(m, rule, ~0ULL, ~0ULL, run, d_rec, d_seq));
    run.publish(totals);
    const uint64_t n = run.h[UT_UNITIGS], bases = run.h[UT_BASES];
    if (n == 0) return TSX_HIP_OK;
    hipStream_t st = m->stream.get();
    std::vector<UnitigRec> rec((size_t)n);
    HIP_TRY(hipMemcpyAsync(rec.data(), d_rec.get(), (size_t)n * sizeof(UnitigRec), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    std::sort(rec.begin(), rec.end(), [](const UnitigRec &x, const UnitigRec &y) { return x.offset < y.offset; });
    uint64_t at = 0;
    for (const UnitigRec &u : rec) {   // the records tile [0, bases)
        if (u.offset != at || u.length > bases - at) { g_last_error = "unitigs: the table is not consistent"; return TSX_HIP_EHIP; }
        at += u.length;
    }
    const uint64_t piece = std::min<uint64_t>(bases, std::max<uint64_t>(WRITE_CHUNK_DEFAULT / 4, run.h[UT_LONGEST]));
    for (int i = 0; i < 2; ++i) { TSX_TRY(pin[i].alloc((size_t)piece)); TSX_TRY(ready[i].create()); }
    // [r0, r1): the records of the piece that starts at record r0
    auto piece_end = [&](uint64_t r0) {
        uint64_t r1 = r0, bytes = 0;
        while (r1 < n && bytes + rec[(size_t)r1].length <= piece) bytes += rec[(size_t)r1++].length;
        return r1;
    };
    auto fetch = [&](uint64_t r0, uint64_t r1, int b) -> int {
        const uint64_t lo = rec[(size_t)r0].offset, hi = rec[(size_t)r1 - 1].offset + rec[(size_t)r1 - 1].length;
        HIP_TRY(hipMemcpyAsync(pin[b].get(), d_seq.get() + lo, (size_t)(hi - lo), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipEventRecord(ready[b].get(), st));
        return TSX_HIP_OK;
    };
    std::vector<uint8_t> text;
    uint64_t r0 = 0, r1 = piece_end(0);
    TSX_TRY(fetch(r0, r1, 0));
    for (int b = 0; r0 < n; b ^= 1) {
        const uint64_t r2 = r1 < n ? piece_end(r1) : r1;
        if (r1 < n) TSX_TRY(fetch(r1, r2, b ^ 1));
        HIP_TRY(hipEventSynchronize(ready[b].get()));
        const uint64_t base = rec[(size_t)r0].offset;
        size_t need = 0;
        for (uint64_t r = r0; r < r1; ++r) need += (size_t)rec[(size_t)r].length + 128;
        text.resize(need);
        size_t w = 0;
        for (uint64_t r = r0; r < r1; ++r) {
            const UnitigRec &u = rec[(size_t)r];
            w += (size_t)snprintf((char *)text.data() + w, 120, ">%llu LN:i:%llu KC:i:%llu km:f:%.1f%s\n", (unsigned long long)r,
                                  (unsigned long long)u.length, (unsigned long long)u.sum_count,
                                  (double)u.sum_count / (double)u.kmers, u.circular ? " CL:i:1" : "");
            memcpy(text.data() + w, pin[b].get() + (u.offset - base), (size_t)u.length);
            w += (size_t)u.length;
            text[w++] = '\n';
        }
        TSX_TRY(write_all(fd, text.data(), w));
        r0 = r1;
        r1 = r2;
    }
    return TSX_HIP_OK;
}

extern "C" int tsx_hip_owner_host(const tsx_hip_map *m, const uint64_t *kmer, int nranks) {
    if (!m || !kmer || nranks < 1) return TSX_HIP_EINVAL;
    uint64_t cx[4];
    if (m->canon) {   // the owner of a strand pair is that of the k-mer its dump reports (dump_kernel)
        tsx_hip_canonical_host(m->p.k, kmer, 1, cx);
        kmer = cx;
    }
    uint64_t z = 0x243F6A8885A308D3ULL;
    for (int t = 0; t < m->p.wk; ++t) {
        uint64_t x = (t == m->p.wk - 1) ? (kmer[t] & m->p.top_mask) : kmer[t];
        z ^= x;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
        z = z ^ (z >> 31);
    }
    return (int)((z >> 32) * (uint64_t)nranks >> 32);
}

extern "C" int tsx_hip_hash_apply(const tsx_hip_map *m, const uint64_t *kmer, uint64_t *key_out) {
    if (!m || !kmer || !key_out) return TSX_HIP_EINVAL;
    std::vector<uint64_t> x(kmer, kmer + m->p.wk);
    x[m->p.wk - 1] &= m->p.top_mask;
    apply_rows(m, m->rows, x.data(), key_out);
    return TSX_HIP_OK;
}
extern "C" int tsx_hip_hash_invert(const tsx_hip_map *m, const uint64_t *key, uint64_t *kmer_out) {
    if (!m || !key || !kmer_out) return TSX_HIP_EINVAL;
    std::vector<uint64_t> x(key, key + m->p.wk);
    x[m->p.wk - 1] &= m->p.top_mask;
    apply_rows(m, m->irows, x.data(), kmer_out);
    return TSX_HIP_OK;
}
extern "C" int tsx_hip_hash_rows(const tsx_hip_map *m, uint64_t *rows_out) {
    if (!m || !rows_out) return TSX_HIP_EINVAL;
    memcpy(rows_out, m->rows.data(), m->rows.size() * 8);
    return TSX_HIP_OK;
}

extern "C" int tsx_hip_lut4_host(int k, int l, uint64_t hash_seed, uint64_t *lut_out) {
    if (!lut_out || k > 32) return TSX_HIP_EINVAL;
    tsx_hip_map t;   // host state only: layout and mapping, no device is touched
    const int rc = derive_layout(&t, k, l, 0, 0, 0, 0);
    if (rc != TSX_HIP_OK) return rc;
    t.seed = hash_seed;
    const int rm = make_mapping(&t);
    if (rm != TSX_HIP_OK) return rm;
    std::vector<uint64_t> lut4;
    make_lut4(&t, lut4);
    memcpy(lut_out, lut4.data(), lut4.size() * 8);
    return TSX_HIP_OK;
}

extern "C" uint64_t tsx_hip_sublist_first(uint32_t nb, uint32_t G, int wg_major, uint32_t b, uint32_t g, uint64_t cap) {
    return sublist_first(sublist_order(nb, G, wg_major), b, g, cap);
}
extern "C" int tsx_hip_level1_sizes_host(tsx_hip_map *m, tsx_hip_level1_shape *shape_out, uint64_t *sizes_out, size_t cap) {
    if (!m || !shape_out) return TSX_HIP_EINVAL;
    const L1Seen &s = m->l1_seen;
    const size_t n = (size_t)s.nb * s.G;
    *shape_out = tsx_hip_level1_shape{s.nb, s.G, s.cpr2, s.wg_major, s.cap};
    if (!sizes_out) return TSX_HIP_OK;
    if (n == 0 || cap < n || (s.at + n) * 8 > m->d_cnt.cap()) return TSX_HIP_EINVAL;
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipStreamSynchronize(m->stream.get()));
    HIP_TRY(hipMemcpy(sizes_out, m->d_cnt.get() + s.at, n * 8, hipMemcpyDeviceToHost));
    return TSX_HIP_OK;
}

// ---- synthetic reads -----------------------------------------------------------
static inline int dec_digits(uint64_t v) { int d = 1; while (v >= 10) { v /= 10; ++d; } return d; }

extern "C" int tsx_hip_synth_fastq_device(uint64_t seed, uint64_t first_read, uint64_t n_reads, int k,
                                          void *dev_out, size_t cap, uint64_t *bytes_out, uint64_t *kmers_out,
                                          uint64_t *polya_kmers_out, int device, void *stream) {
    if (k < 1 || k > 127) return TSX_HIP_EINVAL;
    std::vector<uint64_t> offs(n_reads + 1);
    uint64_t total = 0, kmers = 0, polya = 0;
    for (uint64_t r = 0; r < n_reads; ++r) {
        const uint64_t id = first_read + r;
        const uint32_t nrand = 500u + (uint32_t)(synth_mix(seed, id, 0) % 501u);
        const uint32_t na = 100u + (uint32_t)(synth_mix(seed, id, 1) % 201u);
        const uint64_t L = (uint64_t)nrand + na;
        offs[r] = total;
        total += 4 + dec_digits(id) + 1 + 2 * L + 4;
        if (L >= (uint64_t)k) kmers += L - k + 1;
        if (polya_kmers_out) {
            // all-'A' windows: runs of A inside the random part plus the tail
            uint32_t run = 0;
            for (uint32_t j = 0; j < nrand; ++j) {
                const uint64_t w = synth_mix(seed, id, 2 + (j >> 5));
                if (((w >> (2 * (j & 31))) & 3) == 0) ++run;
                else { if (run >= (uint32_t)k) polya += run - k + 1; run = 0; }
            }
            run += na;
            if (run >= (uint32_t)k) polya += run - k + 1;
        }
    }
    offs[n_reads] = total;
    if (bytes_out) *bytes_out = total;
    if (kmers_out) *kmers_out = kmers;
    if (polya_kmers_out) *polya_kmers_out = polya;
    if (!dev_out) return TSX_HIP_OK;
    if (total > cap) return TSX_HIP_ERANGE;
    if (n_reads == 0) return TSX_HIP_OK;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return TSX_HIP_ENODEVICE;
    HIP_TRY(hipSetDevice(device));
    hipStream_t st = (hipStream_t)stream;
    DevBuf<uint64_t> off;
    TSX_TRY(off.alloc((n_reads + 1) * 8));
    uint64_t *const d_off = off.get();
    int rc = TSX_HIP_OK;
    if (hipMemcpyAsync(d_off, offs.data(), (n_reads + 1) * 8, hipMemcpyHostToDevice, st) != hipSuccess) rc = TSX_HIP_EHIP;
    if (rc == TSX_HIP_OK) {
        const int grid = (int)std::min<uint64_t>(n_reads, 65536);
        hipLaunchKernelGGL(synth_fill_kernel, dim3(grid), dim3(NT), 0, st, seed, first_read, n_reads,
                           (const uint64_t *)d_off, (uint8_t *)dev_out);
        if (hipGetLastError() != hipSuccess) rc = TSX_HIP_EHIP;
    }
    if (hipStreamSynchronize(st) != hipSuccess) rc = TSX_HIP_EHIP;   // (d_off is read until here)
    return rc;
}

// Zipf-skewed reads written straight into device memory (BASELINE config 4; see synth_zipf_kernel).  thr: n_templates
// ascending uint64 thresholds (host).  Sizing call: dev_out == NULL.
extern "C" int tsx_hip_synth_zipf_device(uint64_t seed, uint64_t n_reads, uint32_t read_len, uint32_t n_templates,
                                         const uint64_t *thr, void *dev_out, size_t cap, uint64_t *bytes_out, int device,
                                         void *stream) {
    if (read_len < 1 || read_len > (1u << 20) || n_templates < 1 || !thr) return TSX_HIP_EINVAL;
    std::vector<uint64_t> offs(n_reads + 1);
    uint64_t total = 0;
    for (uint64_t r = 0; r < n_reads; ++r) {
        offs[r] = total;
        total += 2 + dec_digits(r) + 1 + 2 * (uint64_t)read_len + 4;
    }
    offs[n_reads] = total;
    if (bytes_out) *bytes_out = total;
    if (!dev_out) return TSX_HIP_OK;
    if (total > cap) return TSX_HIP_ERANGE;
    if (n_reads == 0) return TSX_HIP_OK;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return TSX_HIP_ENODEVICE;
    HIP_TRY(hipSetDevice(device));
    hipStream_t st = (hipStream_t)stream;
    DevBuf<uint64_t> off, thr_buf;
    TSX_TRY(off.alloc((n_reads + 1) * 8));
    if (thr_buf.alloc((size_t)n_templates * 8) != TSX_HIP_OK) return TSX_HIP_ENOMEM;
    uint64_t *const d_off = off.get(), *const d_thr = thr_buf.get();
    int rc = TSX_HIP_OK;
    if (hipMemcpyAsync(d_off, offs.data(), (n_reads + 1) * 8, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(d_thr, thr, (size_t)n_templates * 8, hipMemcpyHostToDevice, st) != hipSuccess) rc = TSX_HIP_EHIP;
    if (rc == TSX_HIP_OK) {
        const int grid = (int)std::min<uint64_t>(n_reads, 65536);
        hipLaunchKernelGGL(synth_zipf_kernel, dim3(grid), dim3(NT), 0, st, seed, n_reads, read_len, n_templates,
                           (const uint64_t *)d_thr, (const uint64_t *)d_off, (uint8_t *)dev_out);
        if (hipGetLastError() != hipSuccess) rc = TSX_HIP_EHIP;
    }
    if (hipStreamSynchronize(st) != hipSuccess) rc = TSX_HIP_EHIP;   // (both are read until here)
    return rc;
}

// ---- read queries: per-record k-mer stats and the read filter (tsx_query.h) --------------------------------------
static const size_t QUERY_CHUNK_DEFAULT = (size_t)256 << 20;   // text bytes per piece of the host entry points
static const size_t QUERY_PIECE_MAX = (size_t)0xF0000000;      // a piece's line index is 32 bits wide

static bool query_args_ok(const tsx_hip_map *m, uint64_t lower, uint64_t upper) {
    // a shard answers 0 for the k-mers it does not own: its stats would be wrong, not partial
    return m && lower <= upper && m->p.lg == m->p.l;
}

// query_reads_kernel over the start positions [0, own_end) of d_text (n readable bytes), after line_pass.
static int query_launch(tsx_hip_map *m, const uint8_t *d_text, uint64_t n, uint64_t own_end, int head_open,
                        const unsigned long long *d_line_base, uint64_t lower, uint64_t upper, unsigned long long *d_stats,
                        uint64_t cap, hipStream_t st) {
    if (own_end == 0) return TSX_HIP_OK;
    const uint64_t ntiles = (own_end + TILE - 1) / TILE;
    const size_t lut_bytes = m->lut.size() * 8;
    const int grid = (int)std::min<uint64_t>(ntiles, (uint64_t)m->cus * 4);
    const uint32_t lshift = line_shift(m);
    DISPATCH_BR(m, DISPATCH_CANON(m, DISPATCH_WK(m, hipLaunchKernelGGL((query_reads_kernel<WKV, CANV, BRV>), dim3(grid), dim3(NT),
                                                        lut_bytes, st, m->p, d_text, n, own_end, head_open,
                                                        (const uint32_t *)m->d_tile.get(), ntiles, d_line_base, lshift, lower, upper,
                                                        d_stats, (uint64_t)cap, m->qmap_cur))));
    HIP_TRY(hipGetLastError());
    return TSX_HIP_OK;
}

// A device text in windows like tsx_hip_count_fastq_device; the line index of each window continues from a 64-bit base
// on the device (the map's FASTQ scratch: word 0 of d_carry is the scan carry, words 2 and 3 the line base and the
// record count).  `round64`: windows of whole 64-byte words, for the callers that keep one bitmap word per 64 start
// positions.  A quality rule: the bitmap of the whole text first, qmap_cur per window.  Every window: the scan
// carry from zero, the line pass, then per_window(off, own, len, head_open, last, d_base) queues the call's kernels over
// the start positions [off, off + own) (len readable bytes from off), then the base and the record count move on.  The
// record count is left in d_carry word 3.  Queued, not waited for.
template <class PerWindow>
static int device_windows(tsx_hip_map *m, const uint8_t *base, size_t n, bool round64, hipStream_t st, PerWindow per_window) {
    int rc;
    if (m->minq && (rc = build_qmap(m, base, n, st)) != TSX_HIP_OK) return rc;
    const uint16_t *qmap = m->minq ? m->d_qmap.get() : nullptr;
    QmapScope qs(m);
    const uint32_t lpr = m->p.line_mask + 1;
    unsigned long long *d_base = (unsigned long long *)m->d_carry.get() + 2, *d_nrec = d_base + 1;
    HIP_TRY(hipMemsetAsync(d_base, 0, 2 * sizeof(unsigned long long), st));
    const size_t halo = (size_t)m->p.k - 1, WIN = round64 ? (dev_window_bytes() + 63) & ~(size_t)63 : dev_window_bytes();
    auto window_end = [&](bool last, const uint8_t *tail) {
        hipLaunchKernelGGL(query_window_kernel, dim3(1), dim3(64), 0, st, d_base, (const uint32_t *)m->d_carry.get(), last ? 1 : 0,
                           tail, lpr, d_nrec);
    };
    for (size_t off = 0; off < n; off += WIN) {
        const size_t own = std::min(WIN, n - off), len = std::min(own + halo, n - off);
        const int head_open = off > 0 ? -1 : 0;
        const bool last = off + own >= n;
        m->qmap_cur = qmap ? qmap + off / 16 : nullptr;   // (windows start at multiples of 16)
        HIP_TRY(hipMemsetAsync(m->d_carry.get(), 0, sizeof(uint32_t), st));
        if ((rc = line_pass(m, base + off, len, own, head_open, st)) != TSX_HIP_OK) return rc;
        if ((rc = per_window(off, own, len, head_open, last, (const unsigned long long *)d_base)) != TSX_HIP_OK) return rc;
        window_end(last, base + n - 1);
    }
    if (n == 0) {   // (no window has zeroed the carry of an earlier call)
        HIP_TRY(hipMemsetAsync(m->d_carry.get(), 0, sizeof(uint32_t), st));
        window_end(true, nullptr);
    }
    HIP_TRY(hipGetLastError());
    return TSX_HIP_OK;
}

// Behind device_windows and what the call queued after it: waits for the record count.  More records than the caller's
// array holds: TSX_HIP_ERANGE.
static int windows_records(tsx_hip_map *m, size_t cap, size_t *n_records, hipStream_t st) {
    HIP_TRY(hipGetLastError());
    unsigned long long nrec = 0;
    HIP_TRY(hipMemcpyAsync(&nrec, (const unsigned long long *)m->d_carry.get() + 3, sizeof nrec, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (n_records) *n_records = (size_t)nrec;
    return nrec > cap ? TSX_HIP_ERANGE : TSX_HIP_OK;
}

// What the device entry points of the read calls do first: the device, the stream (a caller's, or the map's behind it),
// a lazily cleared table zeroed before anyone reads it, the base rule.  In this order for every call: one that is refused
// for its base rule has zeroed a lazily cleared table on its way, which the next call would have done.
static int device_begin(tsx_hip_map *m, void *stream, hipStream_t &st) {
    HIP_TRY(hipSetDevice(m->device));
    st = pick_stream(m, stream);
    TSX_TRY(ensure_zeroed(m, st));
    return base_rule_ok(m);
}

extern "C" int tsx_hip_query_reads_device(tsx_hip_map *m, const void *dev_text, size_t n, uint64_t lower, uint64_t upper,
                                          void *dev_stats, size_t stats_cap, size_t *n_records, void *stream) {
    if (n_records) *n_records = 0;
    if (!query_args_ok(m, lower, upper) || (!dev_text && n) || ((uintptr_t)dev_text & 15) || (!dev_stats && stats_cap))
        return TSX_HIP_EINVAL;
    hipStream_t st;
    TSX_TRY(device_begin(m, stream, st));
    const uint8_t *base = (const uint8_t *)dev_text;
    unsigned long long *stats = (unsigned long long *)dev_stats;
    if (stats_cap) HIP_TRY(hipMemsetAsync(stats, 0, stats_cap * sizeof(tsx_hip_read_stats), st));
    TSX_TRY(device_windows(m, base, n, false, st,
                           [&](size_t off, size_t own, size_t len, int head_open, bool, const unsigned long long *d_base) {
                               return query_launch(m, base + off, len, own, head_open, d_base, lower, upper, stats, stats_cap, st);
                           }));
    if (stats_cap)
        hipLaunchKernelGGL(query_finalize_kernel, dim3(grid_for(m, stats_cap, 8)), dim3(NT), 0, st, stats, (uint64_t)stats_cap,
                           (const unsigned long long *)m->d_carry.get() + 3, (uint64_t)0);
    return windows_records(m, stats_cap, n_records, st);
}

// Where the compacted output of a piece goes: the caller's buffer (never grown: the *_device entry points check that it
// has the room) or, without one, `own`.
struct OutBuf {
    DevBuf<uint8_t> own;
    uint8_t *out = nullptr; size_t have = 0;   // where it goes, and the room there
    // room for the worst case of a piece cut at `cut`: cut + 1 bytes, rounded up
    int room(hipStream_t st, uint64_t cut) {
        if (cut + 64 > have) {   // (as grow() finds it)
            TSX_TRY(grow(st, own, cut + 64));
            out = own.get(); have = own.cap();
        }
        return TSX_HIP_OK;
    }
};

// Room in `buf` for n + 1 lengths that are scanned in place: one partial sum per SCAN_CHUNK of them lies behind them.
static int scan_room(hipStream_t st, DevBuf<unsigned long long> &buf, uint64_t n) {
    const uint64_t nk = n + 1, nchunks = (nk + SCAN_CHUNK - 1) / SCAN_CHUNK;
    return grow(st, buf, (nk + nchunks + 16) * sizeof(unsigned long long));
}

// The scan of the n + 1 lengths at `off` in place (scan_room behind them): offsets, their total to *total.  Queued.
static int scan_lengths(unsigned long long *off, uint64_t n, unsigned long long *total, hipStream_t st) {
    const uint64_t nk = n + 1, nchunks = (nk + SCAN_CHUNK - 1) / SCAN_CHUNK;
    unsigned long long *chunk = off + nk;
    hipLaunchKernelGGL(u64_chunk_sum_kernel, dim3((uint32_t)nchunks), dim3(SCAN_CHUNK), 0, st, (const unsigned long long *)off, nk, chunk);
    hipLaunchKernelGGL(u64_chunk_scan_kernel, dim3(1), dim3(1024), 0, st, chunk, nchunks, total);
    hipLaunchKernelGGL(u64_scan_kernel, dim3((uint32_t)nchunks), dim3(SCAN_CHUNK), 0, st, off, nk, (const unsigned long long *)chunk);
    HIP_TRY(hipGetLastError());
    return TSX_HIP_OK;
}

// One compaction of a piece: the lengths a call's kernel writes (one or more per record; several arrays may share the
// buffer: the caller hands out entry ranges), scanned in place into offsets, and the output they describe.
struct Compaction {
    DevBuf<unsigned long long> off;
    OutBuf out;
    // room for n + 1 entries and their chunk sums, entry n zeroed (the scan reads it): the array, for the call's kernel
    int lengths(hipStream_t st, uint64_t n, unsigned long long *&len) {
        TSX_TRY(scan_room(st, off, n));
        HIP_TRY(hipMemsetAsync(off.get() + n, 0, sizeof(unsigned long long), st));
        len = off.get();
        return TSX_HIP_OK;
    }
    // What both copy steps are: room in out for a piece cut at `cut`, the scan (the total goes to *total), then `kern` moves
    // d_text[0, cut) into out by what `by` holds -- the copy grid covers the worst case, lanes past the total fall through.
    // Queued, not waited for.
    template <class Kernel>
    int copy(Kernel kern, tsx_hip_map *m, const uint8_t *d_text, uint64_t cut, const unsigned long long *by, uint64_t n,
             unsigned long long *total, hipStream_t st) {
        TSX_TRY(out.room(st, cut));
        TSX_TRY(scan_lengths(off.get(), n, total, st));
        hipLaunchKernelGGL(kern, dim3(grid_for(m, (cut + 16) / 16 + 64, 8)), dim3(NT), 0, st, d_text, cut, by,
                           (const unsigned long long *)off.get(), n, out.out, (uint64_t)out.have);
        HIP_TRY(hipGetLastError());
        return TSX_HIP_OK;
    }
    // by the record spans; by segments, each with its source in src
    int copy_spans(tsx_hip_map *m, const uint8_t *d_text, uint64_t cut, const unsigned long long *span, uint64_t n,
                   unsigned long long *total, hipStream_t st) { return copy(filter_copy_kernel, m, d_text, cut, span, n, total, st); }
    int copy_segments(tsx_hip_map *m, const uint8_t *d_text, uint64_t cut, const unsigned long long *src, uint64_t n,
                      unsigned long long *total, hipStream_t st) { return copy(trim_copy_kernel, m, d_text, cut, src, n, total, st); }
};

// Scratch of one query / filter call that works on pieces.
struct QueryBufs {
    DevBuf<unsigned long long> stats;
    Compaction c;      // the filter's kept lengths and its output
    PieceBufs p;
    explicit QueryBufs(hipStream_t s) : p(s) {}
};

// The query half: the stats of the records [0, nrec) of d_text[0, cut) in b.stats, after a line pass over a text that
// starts with [0, cut) (the tile line counts).  Queued, not waited for.
static int query_records(tsx_hip_map *m, QueryBufs &b, const uint8_t *d_text, uint64_t cut, uint64_t nrec, uint64_t lower,
                         uint64_t upper, hipStream_t st) {
    TSX_TRY(grow(st, b.stats, nrec * sizeof(tsx_hip_read_stats)));
    HIP_TRY(hipMemsetAsync(b.stats.get(), 0, nrec * sizeof(tsx_hip_read_stats), st));
    QmapScope qs(m);
    TSX_TRY(piece_qmap(m, d_text, cut, st));
    TSX_TRY(query_launch(m, d_text, cut, cut, 0, b.p.info.get() + 4, lower, upper, b.stats.get(), nrec, st));
    hipLaunchKernelGGL(query_finalize_kernel, dim3(grid_for(m, nrec, 8)), dim3(NT), 0, st, b.stats.get(), nrec,
                       (const unsigned long long *)nullptr, nrec);
    HIP_TRY(hipGetLastError());
    return TSX_HIP_OK;
}

// One piece: piece_front, then -- when it holds a whole record -- the stats of its records [0, nrec) in b.stats, queued
// and not waited for.  Not last and no whole record: nrec = 0, nothing queried.
static int query_piece(tsx_hip_map *m, QueryBufs &b, const uint8_t *d_text, uint64_t len, bool last, uint64_t lower,
                       uint64_t upper, bool spans, hipStream_t st, uint64_t &cut, uint64_t &nrec, bool &open) {
    TSX_TRY(piece_front(m, b.p, d_text, len, last, spans, cut, nrec, open));
    if (nrec == 0) return TSX_HIP_OK;
    return query_records(m, b, d_text, cut, nrec, lower, upper, st);
}

// The filter behind query_piece: kept lengths, their scan (total -> info[3], kept records -> info[5]), the compaction
// into b.c.out.  Queued, not waited for.
static int filter_piece(tsx_hip_map *m, QueryBufs &b, const uint8_t *d_text, uint64_t cut, uint64_t nrec, bool open,
                        const tsx_hip_filter_rule &rule, hipStream_t st) {
    unsigned long long *koff, *const info = b.p.info.get();
    const unsigned long long *span = b.p.rspan.get();
    TSX_TRY(b.c.lengths(st, nrec, koff));
    hipLaunchKernelGGL(filter_len_kernel, dim3(grid_for(m, nrec, 8)), dim3(NT), 0, st, (const unsigned long long *)b.stats.get(),
                       span, nrec, rule.min_in_range, (uint64_t)rule.fraction_ppm, rule.invert,
                       open ? 1 : 0, koff, info + 5);
    return b.c.copy_spans(m, d_text, cut, span, nrec, info + 3, st);
}

static bool rule_ok(const tsx_hip_filter_rule *r) {
    return r && r->lower <= r->upper && r->fraction_ppm <= 1000000u;
}

// What a host call does first: its piece size (0: the default; `piece_cap`: at most the map's TSX_HIP_PIECE_BYTES, which
// only the median and the sketch calls honour -- DESIGN.md §3), the device, the order behind a caller's stream, the base rule, the table.
static int pieces_begin(tsx_hip_map *m, size_t &chunk_bytes, bool piece_cap) {
    if (!chunk_bytes) chunk_bytes = QUERY_CHUNK_DEFAULT;
    if (piece_cap && m->piece_fixed) chunk_bytes = std::min(chunk_bytes, m->piece);
    chunk_bytes = std::min(chunk_bytes, QUERY_PIECE_MAX);
    HIP_TRY(hipSetDevice(m->device));
    join_foreign(m, false);
    TSX_TRY(base_rule_ok(m));
    return ensure_zeroed(m, m->stream.get());
}

// The piece text[0, len) to the device.  Queued, not waited for.
static int piece_upload(PieceBufs &p, const char *text, size_t len) {
    TSX_TRY(grow(p.st, p.text, len + 256));
    HIP_TRY(hipMemcpyAsync(p.text.get(), text, len, hipMemcpyHostToDevice, p.st));
    return TSX_HIP_OK;
}

// A piece that holds no whole record (a record longer than the piece) doubles, up to the `rest` of its text.
static int piece_longer(size_t &len, size_t rest) {
    if (len >= QUERY_PIECE_MAX) { g_last_error = "a record longer than 3.75 GiB"; return TSX_HIP_EINVAL; }
    len = std::min(std::min(2 * len, rest), QUERY_PIECE_MAX);
    return TSX_HIP_OK;
}

// The driver of the single-end host calls: the text in pieces cut at record boundaries, chunk_bytes at a time; a piece
// without a whole record grows until it holds one.  Every piece goes to the device and through
//   work(d_text, len, last, cut, nrec, open)     the call's *_piece: waits once, for the cut; the rest queued
//   deliver(off, rec_base, cut, nrec, open)      the results of text[off, off + cut), records [rec_base, rec_base + nrec)
// and the next one starts at the cut.  rec_base: the records of the pieces delivered (of a failed delivery too).
template <class Work, class Deliver>
static int host_pieces(tsx_hip_map *m, PieceBufs &p, const char *text, size_t n, size_t chunk_bytes, bool piece_cap,
                       uint64_t &rec_base, Work work, Deliver deliver) {
    TSX_TRY(pieces_begin(m, chunk_bytes, piece_cap));
    TSX_TRY(p.init());
    for (size_t off = 0; off < n;) {
        size_t len = std::min(chunk_bytes, n - off);
        uint64_t cut = 0, nrec = 0;
        bool open = false;
        for (;;) {
            const bool last = off + len == n;
            TSX_TRY(piece_upload(p, text + off, len));
            TSX_TRY(work((const uint8_t *)p.text.get(), (uint64_t)len, last, cut, nrec, open));
            if (nrec || last) break;
            TSX_TRY(piece_longer(len, n - off));
        }
        const int rc = deliver(off, rec_base, cut, nrec, open);
        rec_base += nrec;
        off += cut;
        if (rc != TSX_HIP_OK) return rc;
    }
    return TSX_HIP_OK;
}

// Delivery to a caller's array of `cap` records: the records [rec_base, rec_base + nrec) of a piece, while they fit.
template <class T>
static int deliver_records(T *out, size_t cap, uint64_t rec_base, const void *d_rec, uint64_t nrec, hipStream_t st) {
    if (rec_base >= cap || !nrec) return TSX_HIP_OK;
    HIP_TRY(hipMemcpyAsync(out + rec_base, d_rec, std::min<uint64_t>(nrec, cap - rec_base) * sizeof(T), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return TSX_HIP_OK;
}

// Delivery to a file, behind the device: the output of piece i waits in a pinned buffer and is written to fd while the
// device works on piece i + 1.  Declare it in FRONT of the scratch that waits for the stream when the call ends.
struct WriteBehind {
    PinBuf<uint8_t> h_out;
    int fd = -1;
    uint64_t pending = 0, bytes = 0;   // bytes that wait in h_out; bytes written
    // what waits, to the file
    int flush() {
        if (fd < 0 || !pending) return TSX_HIP_OK;
        TSX_TRY(write_all(fd, h_out.get(), pending));
        bytes += pending;
        pending = 0;
        return TSX_HIP_OK;
    }
    // `total` bytes at d_out into the pinned buffer: queued, the caller waits.  A piece cut at `cut` writes cut + 1 at most.
    int stage(const uint8_t *d_out, uint64_t total, uint64_t cut, const char *what, hipStream_t st) {
        if (total > cut + 1) { g_last_error = std::string(what) + " output larger than its piece"; return TSX_HIP_EHIP; }
        // (no wait: the copy that last filled it has been waited for, and written out by flush())
        if (h_out.reserve(nullptr, total, total + total / 8 + 4096) != TSX_HIP_OK) return TSX_HIP_ENOMEM;
        if (total) HIP_TRY(hipMemcpyAsync(h_out.get(), d_out, total, hipMemcpyDeviceToHost, st));
        pending = total;
        return TSX_HIP_OK;
    }
    // One round (a piece; a round of pairs) of a call with the outputs w[0, nout) (fd < 0: not wanted), behind the kernels
    // that leave the outputs on the device and their sizes and counters in the call's words.  In two steps, so that a
    // call can look at the words in between.
    // Step 1: nwords of d_words to their pinned copy.  The previous round's outputs are written to their files between
    // the event record and the event wait: while the device works on this round.
    static int words_back(WriteBehind *w, int nout, const unsigned long long *d_words, unsigned long long *h_words, size_t nwords,
                          hipEvent_t ev, hipStream_t st) {
        HIP_TRY(hipMemcpyAsync(h_words, d_words, nwords * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipEventRecord(ev, st));
        for (int i = 0; i < nout; ++i) TSX_TRY(w[i].flush());
        HIP_TRY(hipEventSynchronize(ev));
        return TSX_HIP_OK;
    }
    // Step 2: output i is staged from d_out[i], size[i] bytes of a piece cut at cut[i]; a wait when there are bytes; then
    // the nzero words at d_zero start from zero again (sizes and counters are per round).
    static int stage_all(WriteBehind *w, int nout, const uint8_t *const *d_out, const unsigned long long *size, const uint64_t *cut,
                         const char *what, unsigned long long *d_zero, size_t nzero, hipStream_t st) {
        bool any = false;
        for (int i = 0; i < nout; ++i) {
            if (w[i].fd < 0) continue;
            TSX_TRY(w[i].stage(d_out[i], size[i], cut[i], what, st));
            any |= size[i] != 0;
        }
        if (any) HIP_TRY(hipStreamSynchronize(st));
        HIP_TRY(hipMemsetAsync(d_zero, 0, nzero * sizeof(unsigned long long), st));
        return TSX_HIP_OK;
    }
    // One piece of a single-end call: the output at d_out, its size in info[3] and `ncount` counters in info[5..], which
    // are added to count[].
    int piece(PieceBufs &p, const uint8_t *d_out, uint64_t cut, int ncount, uint64_t *count, const char *what) {
        const unsigned long long *h_info = p.h_info.get();
        TSX_TRY(words_back(this, 1, p.info.get() + 3, p.h_info.get() + 3, 2 + ncount, p.ev.get(), p.st));
        TSX_TRY(stage_all(this, 1, &d_out, h_info + 3, &cut, what, p.info.get() + 5, ncount, p.st));
        for (int i = 0; i < ncount; ++i) count[i] += h_info[5 + i];
        return TSX_HIP_OK;
    }
};

// The last step of the calls that leave one piece's output in a caller's device buffer: info[3, 3 + nwords) to the pinned
// copy (h: set once they are there), the wait, and a total above cut + 1 refused.
static int piece_words(PieceBufs &p, int nwords, uint64_t cut, const char *what, const unsigned long long *&h) {
    HIP_TRY(hipMemcpyAsync(p.h_info.get() + 3, p.info.get() + 3, nwords * sizeof(unsigned long long), hipMemcpyDeviceToHost, p.st));
    HIP_TRY(hipStreamSynchronize(p.st));
    h = p.h_info.get();
    if (h[3] > cut + 1) { g_last_error = std::string(what) + " output larger than its text"; return TSX_HIP_EHIP; }
    return TSX_HIP_OK;
}

// Query and filter: the pieces of host_pieces.  stats mode (fd < 0): each piece's stats go to stats_out[rec_base ..]
// while they fit.  filter mode: write-behind to fd.
static int query_host(tsx_hip_map *m, const char *text, size_t n, uint64_t lower, uint64_t upper, size_t chunk_bytes,
                      tsx_hip_read_stats *stats_out, size_t stats_cap, size_t *n_records, const tsx_hip_filter_rule *rule,
                      int fd, uint64_t *kept_out, uint64_t *bytes_out) {
    hipStream_t st = m->stream.get();
    WriteBehind wb;
    wb.fd = fd;
    QueryBufs b(st);
    uint64_t rec_base = 0, kept = 0;
    int rc = host_pieces(m, b.p, text, n, chunk_bytes, false, rec_base,
        [&](const uint8_t *d_text, uint64_t len, bool last, uint64_t &cut, uint64_t &nrec, bool &open) {
            return query_piece(m, b, d_text, len, last, lower, upper, rule != nullptr, st, cut, nrec, open);
        },
        [&](size_t, uint64_t base, uint64_t cut, uint64_t nrec, bool open) -> int {
            if (!rule) return deliver_records(stats_out, stats_cap, base, b.stats.get(), nrec, st);
            if (!nrec) return TSX_HIP_OK;
            TSX_TRY(filter_piece(m, b, b.p.text.get(), cut, nrec, open, *rule, st));
            return wb.piece(b.p, b.c.out.out, cut, 1, &kept, "filter");
        });
    if (rc == TSX_HIP_OK) rc = wb.flush();
    if (n_records) *n_records = (size_t)rec_base;
    if (kept_out) *kept_out = kept;
    if (bytes_out) *bytes_out = wb.bytes;
    if (rc == TSX_HIP_OK && !rule && rec_base > stats_cap) rc = TSX_HIP_ERANGE;
    return rc;
}

extern "C" int tsx_hip_query_reads_host(tsx_hip_map *m, const char *text, size_t n, uint64_t lower, uint64_t upper,
                                        tsx_hip_read_stats *stats_out, size_t stats_cap, size_t *n_records, size_t chunk_bytes) {
    if (n_records) *n_records = 0;
    if (!query_args_ok(m, lower, upper) || (!text && n) || (!stats_out && stats_cap)) return TSX_HIP_EINVAL;
    return query_host(m, text, n, lower, upper, chunk_bytes, stats_out, stats_cap, n_records, nullptr, -1, nullptr, nullptr);
}

extern "C" int tsx_hip_filter_reads_host(tsx_hip_map *m, const char *text, size_t n, const tsx_hip_filter_rule *rule, int fd,
                                         size_t chunk_bytes, uint64_t *kept_out, uint64_t *bytes_out) {
    if (kept_out) *kept_out = 0;
    if (bytes_out) *bytes_out = 0;
    if (!rule_ok(rule) || !query_args_ok(m, rule->lower, rule->upper) || (!text && n) || fd < 0) return TSX_HIP_EINVAL;
    return query_host(m, text, n, rule->lower, rule->upper, chunk_bytes, nullptr, 0, nullptr, rule, fd, kept_out, bytes_out);
}

extern "C" int tsx_hip_filter_reads_device(tsx_hip_map *m, const void *dev_text, size_t n, const tsx_hip_filter_rule *rule,
                                           void *dev_out, size_t out_cap, size_t *out_bytes, uint64_t *kept_out, void *stream) {
    if (out_bytes) *out_bytes = 0;
    if (kept_out) *kept_out = 0;
    if (!rule_ok(rule) || !query_args_ok(m, rule->lower, rule->upper) || (!dev_text && n) || ((uintptr_t)dev_text & 15) ||
        !dev_out || ((uintptr_t)dev_out & 15) || n >= QUERY_PIECE_MAX)
        return TSX_HIP_EINVAL;
    if (out_cap < n + 64) return TSX_HIP_ERANGE;
    hipStream_t st;
    TSX_TRY(device_begin(m, stream, st));
    QueryBufs b(st);
    int rc = b.p.init();
    b.c.out.out = (uint8_t *)dev_out; b.c.out.have = out_cap;   // the compaction writes the caller's buffer (never grown)
    uint64_t cut = 0, nrec = 0;
    bool open = false;
    const unsigned long long *h = nullptr;
    if (rc == TSX_HIP_OK) rc = query_piece(m, b, (const uint8_t *)dev_text, n, true, rule->lower, rule->upper, true, st, cut, nrec, open);
    if (rc == TSX_HIP_OK && nrec) rc = filter_piece(m, b, (const uint8_t *)dev_text, cut, nrec, open, *rule, st);
    if (rc == TSX_HIP_OK && nrec) rc = piece_words(b.p, 3, cut, "filter", h);
    if (out_bytes && h) *out_bytes = (size_t)h[3];
    if (kept_out && h) *kept_out = h[5];
    return rc;
}

// ---- sequence queries: the sequences of a wrapped FASTA against the table (tsx_seq.h) ------------------------------
struct tsx_hip_seq_result {
    std::vector<tsx_hip_seq_stats> stats;
    std::string names;
    std::vector<uint64_t> name_off{0};
    std::vector<tsx_hip_seq_interval> iv;
    uint64_t window = 0;                 // the track's window; 0: no track
    std::vector<tsx_hip_seq_bin> bins;   // the bins of sequence i: [first[i], first[i + 1])
    std::vector<uint64_t> first{0};
};

static const size_t SEQ_NAME_BATCH = 65536;   // headers described per launch of seq_names_kernel
// Fragments the device holds at a time (TSX_HIP_SEQ_FRAGS: tests make the buffer wrap): whole tiles' worth.
static size_t seq_frag_cap() {
    size_t v = (size_t)1 << 22;
    if (const char *e = getenv("TSX_HIP_SEQ_FRAGS")) { const long long x = atoll(e); if (x > 0) v = (size_t)x; }
    return std::max<size_t>(v / SEQ_TILE_FRAGS, 1) * SEQ_TILE_FRAGS;
}

// One call's state.  The carry of sequence identity across pieces lives on the host, next to the copy of the unwrap's
// carry words read back after every piece (each piece waits for its record count anyway): where the text stands, whether
// the open record has sequence, the bases carried; the sequences started are res->stats, the bases so far of the open one
// its length there; the pending name is the last header that has not yet met a sequence byte.
struct SeqRun {
    tsx_hip_map *m;
    hipStream_t st;
    uint64_t lower, upper;
    bool want_missing;
    uint64_t window;   // > 0: the track call -- seq_track_kernel in place of seq_stats_kernel, the stats out of the bins
    tsx_hip_seq_result *res;
    uint32_t where = 0, q = 0, nb = 0;
    std::string pend;
    bool pend_open = false, pend_has = false;
    std::vector<std::string> new_names;
    std::vector<uint32_t> hp;
    std::vector<SeqName> ent;
    std::vector<tsx_hip_seq_stats> rows_h;
    std::vector<tsx_hip_seq_interval> frag_h;
    std::vector<tsx_hip_seq_bin> bins_h;
    DevBuf<unsigned long long> rows, frag, bins, row_of;
    DevBuf<uint32_t> hpos;
    DevBuf<SeqName> hent;
    // words of its own, on the device and pinned: 0 = fragments of a launch, 1 = headers of a piece, 2 and 3 = the three
    // 32-bit carry words of the unwrap read back (pinned only); p.info word 4 stays the zero line base of the kernels
    DevBuf<unsigned long long> words;
    PinBuf<unsigned long long> h_words;
    PieceBufs p;   // (last: its destructor waits for the stream before the buffers above go)
    int init() {
        TSX_TRY(words.alloc(4 * sizeof(unsigned long long)));
        TSX_TRY(h_words.alloc(4 * sizeof(unsigned long long)));
        return p.init();
    }
    SeqRun(tsx_hip_map *mm, hipStream_t s, uint64_t lo, uint64_t up, bool miss, uint64_t win, tsx_hip_seq_result *r)
        : m(mm), st(s), lower(lo), upper(up), want_missing(miss), window(win), res(r), p(s) { r->window = win; }
};

static int seq_fail(const char *why) { g_last_error = why; return TSX_HIP_EINVAL; }
static int seq_args_ok(const tsx_hip_map *m, uint64_t lower, uint64_t upper) {
    if (!m) return TSX_HIP_EINVAL;
    if (lower > upper) return seq_fail("sequence query: lower > upper");
    if (m->p.lg != m->p.l) return seq_fail("sequence query: a map created with shard_bits > 0");
    if (m->minq) return seq_fail("sequence query: min_qual_char needs FASTQ records (a FASTA text has no quality line)");
    return TSX_HIP_OK;
}

static std::string seq_name_of(const std::string &raw) {
    size_t cut = raw.find_first_of(" \t");
    if (cut == std::string::npos) cut = raw.size();
    return raw.substr(0, std::min<size_t>(cut, TSX_HIP_SEQ_NAME_MAX));
}

// The names of the sequences that START in the piece d_text[0, n), in order, into R.new_names; the pending name moves on.
static int seq_names_piece(SeqRun &R, const uint8_t *d_text, uint64_t n) {
    tsx_hip_map *m = R.m;
    hipStream_t st = R.st;
    R.new_names.clear();
    unsigned long long *d_count = R.words.get() + 1, *h_count = R.h_words.get() + 1;
    uint64_t cap = std::max<uint64_t>(n / 64 + 1024, SEQ_NAME_BATCH + 1), count = 0;
    for (int pass = 0; pass < 2; ++pass) {
        TSX_TRY(grow(st, R.hpos, cap * 4));
        HIP_TRY(hipMemsetAsync(d_count, 0, sizeof(unsigned long long), st));
        hipLaunchKernelGGL(seq_heads_kernel, dim3(grid_for(m, (n + 15) / 16, 8)), dim3(NT), 0, st, d_text, n, R.where == 0 ? 1 : 0,
                           R.hpos.get(), d_count, cap);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h_count, d_count, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        count = *h_count;
        if (count <= cap) break;
        cap = count;
    }
    const bool head = R.where == 1 || (R.where == 0 && R.q == 0);
    R.hp.assign(head ? 1 : 0, SEQ_NOPOS);
    R.hp.resize(R.hp.size() + count);
    if (count) HIP_TRY(hipMemcpy(R.hp.data() + (head ? 1 : 0), R.hpos.get(), count * 4, hipMemcpyDeviceToHost));
    std::sort(R.hp.begin() + (head ? 1 : 0), R.hp.end());
    for (size_t at = 0; at < R.hp.size(); at += SEQ_NAME_BATCH) {
        const size_t nb = std::min(SEQ_NAME_BATCH, R.hp.size() - at);
        TSX_TRY(grow(st, R.hent, nb * sizeof(SeqName)));
        HIP_TRY(hipMemcpyAsync(R.hpos.get(), R.hp.data() + at, nb * 4, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(seq_names_kernel, dim3(grid_for(m, nb, 8)), dim3(NT), 0, st, d_text, n, (const uint32_t *)R.hpos.get(),
                           (uint64_t)nb, R.where == 1 ? 1 : 0, R.hent.get());
        HIP_TRY(hipGetLastError());
        R.ent.resize(nb);
        HIP_TRY(hipMemcpyAsync(R.ent.data(), R.hent.get(), nb * sizeof(SeqName), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (size_t i = 0; i < nb; ++i) {
            const SeqName &e = R.ent[i];
            const std::string raw((const char *)e.raw, std::min<uint32_t>(e.len, SEQ_NAME_RAW));
            if (R.hp[at + i] == SEQ_NOPOS) {   // the head of the piece: the pending header's line goes on, or ends here
                if (R.where == 1) {
                    if (R.pend.size() < (size_t)SEQ_NAME_RAW) R.pend.append(raw, 0, SEQ_NAME_RAW - R.pend.size());
                    R.pend_open = (e.flags & SEQ_F_OPEN) != 0;
                    if (R.pend_open) continue;
                }
                if (e.flags & SEQ_F_SEQ) {
                    R.new_names.push_back(R.pend_has ? seq_name_of(R.pend) : std::string());
                    R.pend_has = false;
                } else if (!(e.flags & SEQ_F_END)) {
                    R.pend_has = false;   // (the next header takes over)
                }
                continue;
            }
            if (e.flags & (SEQ_F_OPEN | SEQ_F_END)) {   // (the last header of the piece: pending)
                R.pend = raw;
                R.pend_open = (e.flags & SEQ_F_OPEN) != 0;
                R.pend_has = true;
            } else {
                if (e.flags & SEQ_F_SEQ) R.new_names.push_back(seq_name_of(raw));
                R.pend_has = false;
            }
        }
    }
    if (!R.pend_has) { R.pend.clear(); R.pend_open = false; }
    return TSX_HIP_OK;
}

// Sorted fragments of one launch behind the intervals so far: fragments of one sequence that abut in windows merge.
static void seq_merge_fragments(SeqRun &R) {
    std::sort(R.frag_h.begin(), R.frag_h.end(), [](const tsx_hip_seq_interval &a, const tsx_hip_seq_interval &b) {
        return a.seq != b.seq ? a.seq < b.seq : a.start < b.start;
    });
    const uint64_t k = (uint64_t)R.m->p.k;
    std::vector<tsx_hip_seq_interval> &iv = R.res->iv;
    for (const tsx_hip_seq_interval &f : R.frag_h) {
        if (!iv.empty() && iv.back().seq == f.seq && f.start + k == iv.back().end + 1) iv.back().end = f.end;
        else iv.push_back(f);
    }
    R.frag_h.clear();
}

// ---- coverage tracks: the bins of a piece (tsx_track.h) ------------------------------------------------------------
static uint64_t track_rows_of(uint64_t off, uint64_t len, uint64_t W) { return (off + len + W - 1) / W - off / W; }

// The track kernel over the unwrapped piece two[0, ub) of nrec records: the rows per record and their prefix, the zeroed
// bin rows (bounded by ub / W + nrec + 1 without a wait), the kernel, the finalize.  Queued, not waited for.
static int track_launch(SeqRun &R, const uint8_t *two, uint64_t ub, uint64_t nrec, uint64_t row0_off) {
    tsx_hip_map *m = R.m;
    hipStream_t st = R.st;
    const uint64_t W = R.window, cap = ub / W + nrec + 1;
    TSX_TRY(scan_room(st, R.row_of, nrec));
    TSX_TRY(grow(st, R.bins, cap * sizeof(tsx_hip_seq_bin)));
    HIP_TRY(hipMemsetAsync(R.bins.get(), 0, cap * sizeof(tsx_hip_seq_bin), st));
    const unsigned long long *span = R.p.rspan.get(), *d_base = R.p.info.get() + 4;
    unsigned long long *row_of = R.row_of.get(), *d_total = R.words.get();
    hipLaunchKernelGGL(track_rows_kernel, dim3(grid_for(m, nrec + 1, 8)), dim3(NT), 0, st, span, nrec, W, row0_off, row_of);
    TSX_TRY(scan_lengths(row_of, nrec, d_total, st));
    const uint64_t ntiles = (ub + TILE - 1) / TILE;
    const size_t lut_bytes = m->lut.size() * 8;
    const int grid = (int)std::min<uint64_t>(ntiles, (uint64_t)m->cus * 4);
    const uint32_t magic = (uint32_t)(((uint64_t)1 << 32) / W + 1);
    DISPATCH_BR(m, DISPATCH_CANON(m, DISPATCH_WK(m, hipLaunchKernelGGL((seq_track_kernel<WKV, CANV, BRV>), dim3(grid), dim3(NT), lut_bytes,
                                                        st, m->p, two, ub, (const uint32_t *)m->d_tile.get(), ntiles, d_base, R.lower,
                                                        R.upper, R.bins.get(), cap, nrec, span, (const unsigned long long *)row_of, W,
                                                        magic, row0_off, row0_off / W))));
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(track_finalize_kernel, dim3(grid_for(m, cap, 8)), dim3(NT), 0, st, R.bins.get(), (const unsigned long long *)d_total, cap);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(R.h_words.get(), d_total, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    return TSX_HIP_OK;
}

static void track_combine(tsx_hip_seq_bin &a, const tsx_hip_seq_bin &b) {
    if (b.kmers) a.min_count = a.kmers ? std::min(a.min_count, b.min_count) : b.min_count;
    a.max_count = std::max(a.max_count, b.max_count);
    a.kmers += b.kmers; a.present += b.present; a.sum_count += b.sum_count;
}

// Behind the piece's wait (R.rows_h holds the lengths, the device total is in R.h_words): the bin rows of the piece come
// back, every record's stats are summed out of its rows, and the rows join the result -- record 0 of a piece that goes on
// with the open sequence lands on that sequence's bins from bin row0_off / W on (rows it has already are combined, the
// carried bases start in them), every other record appends.
static int track_merge(SeqRun &R, uint64_t nrec, bool q_in, uint64_t carried, uint64_t row0_off) {
    const uint64_t W = R.window;
    tsx_hip_seq_result &res = *R.res;
    uint64_t total = 0;
    for (uint64_t r = 0; r < nrec; ++r) total += track_rows_of(r == 0 ? row0_off : 0, R.rows_h[r].length + (r == 0 ? carried : 0), W);
    if (total != *R.h_words.get() || total > R.bins.cap() / sizeof(tsx_hip_seq_bin)) {
        g_last_error = "sequence track: the host and the device disagree on the bin rows of a piece";
        return TSX_HIP_EHIP;
    }
    R.bins_h.resize(total);
    if (total) HIP_TRY(hipMemcpy(R.bins_h.data(), R.bins.get(), total * sizeof(tsx_hip_seq_bin), hipMemcpyDeviceToHost));
    size_t at = 0;
    for (uint64_t r = 0; r < nrec; ++r) {
        const uint64_t off = r == 0 ? row0_off : 0;
        const uint64_t rows = track_rows_of(off, R.rows_h[r].length + (r == 0 ? carried : 0), W);
        tsx_hip_seq_bin sum = {0, 0, 0, 0, 0};
        for (uint64_t i = 0; i < rows; ++i) track_combine(sum, R.bins_h[at + i]);
        tsx_hip_seq_stats &s = R.rows_h[r];
        s.kmers = sum.kmers; s.present = sum.present; s.min_count = sum.min_count; s.sum_count = sum.sum_count;
        if (r == 0 && q_in) {
            const size_t seq0 = (size_t)res.first[res.first.size() - 2];   // where the open sequence's bins start
            for (uint64_t i = 0; i < rows; ++i) {
                const size_t g = seq0 + (size_t)(off / W + i);
                if (g < res.bins.size()) track_combine(res.bins[g], R.bins_h[at + i]);
                else res.bins.push_back(R.bins_h[at + i]);
            }
            res.first.back() = res.bins.size();
        } else {
            res.bins.insert(res.bins.end(), R.bins_h.begin() + at, R.bins_h.begin() + at + rows);
            res.first.push_back(res.bins.size());
        }
        at += rows;
    }
    return TSX_HIP_OK;
}

// One piece of the wrapped text, behind the carry: names, the unwrap, the record scan of the two-line text (the one wait
// for its record count), the stats kernel (per fragment-buffer's worth of tiles when the missing runs are wanted), and
// the rows of the piece merged into the result.  A track call (R.window) runs the track kernel in place of the stats kernel
// and fills the piece's rows from its bins (track_launch, track_merge).
static int seq_piece(SeqRun &R, const uint8_t *d_text, uint64_t n) {
    if (n == 0) return TSX_HIP_OK;
    tsx_hip_map *m = R.m;
    hipStream_t st = R.st;
    TSX_TRY(seq_names_piece(R, d_text, n));
    const size_t ub = fa_bound(n, m->p.k);
    TSX_TRY(grow(st, m->d_fa_out, ub + FA_TAIL));
    TSX_TRY(fasta_unwrap(d_text, n, m->d_fa_carry.get(), (uint32_t)m->p.k - 1u, m->d_fa_ws, m->d_fa_out.get(), ub + FA_TAIL, m->cus, st));
    const uint8_t *two = m->d_fa_out.get();
    unsigned long long *h_carry = R.h_words.get() + 2;   // (three 32-bit words in two of its own)
    HIP_TRY(hipMemcpyAsync(h_carry, m->d_fa_carry.get(), 12, hipMemcpyDeviceToHost, st));
    uint64_t cut = 0, nrec = 0;
    bool open = false;
    TSX_TRY(piece_front(m, R.p, two, ub, true, true, cut, nrec, open));   // (waits)
    const uint32_t q_in = R.q, nb_in = R.q ? R.nb : 0u;
    uint32_t cw[3];
    memcpy(cw, h_carry, 12);
    R.where = cw[0]; R.q = cw[1] ? 1u : 0u; R.nb = cw[2];
    std::vector<tsx_hip_seq_stats> &S = R.res->stats;
    if (nrec < q_in || nrec - q_in != R.new_names.size() || (q_in && S.empty())) {
        g_last_error = "sequence query: the name pass and the unwrap disagree on the sequences of a piece";
        return TSX_HIP_EHIP;
    }
    if (nrec == 0) return TSX_HIP_OK;
    const uint64_t seq_base = S.size() - q_in, row0_off = q_in ? S.back().length - nb_in : 0;
    TSX_TRY(grow(st, R.rows, nrec * sizeof(tsx_hip_seq_stats)));
    HIP_TRY(hipMemsetAsync(R.rows.get(), 0, nrec * sizeof(tsx_hip_seq_stats), st));
    const uint64_t ntiles = (ub + TILE - 1) / TILE;
    const size_t lut_bytes = m->lut.size() * 8;
    const unsigned long long *span = R.p.rspan.get(), *d_base = R.p.info.get() + 4;
    unsigned long long *d_nfrag = R.words.get(), *h_nfrag = R.h_words.get();
    const size_t frag_cap = R.want_missing ? seq_frag_cap() : 0;
    if (R.want_missing) TSX_TRY(grow(st, R.frag, frag_cap * sizeof(tsx_hip_seq_interval)));
    const uint64_t step = R.want_missing ? frag_cap / SEQ_TILE_FRAGS : ntiles;
    if (R.window) TSX_TRY(track_launch(R, two, ub, nrec, row0_off));
    for (uint64_t t0 = 0; t0 < ntiles && !R.window; t0 += step) {
        const uint64_t t1 = std::min(ntiles, t0 + step);
        const int grid = (int)std::min<uint64_t>(t1 - t0, (uint64_t)m->cus * 4);
        unsigned long long *d_frag = R.want_missing ? R.frag.get() : (unsigned long long *)nullptr;
        if (R.want_missing) HIP_TRY(hipMemsetAsync(d_nfrag, 0, sizeof(unsigned long long), st));
        DISPATCH_BR(m, DISPATCH_CANON(m, DISPATCH_WK(m, hipLaunchKernelGGL((seq_stats_kernel<WKV, CANV, BRV>), dim3(grid), dim3(NT),
                                                            lut_bytes, st, m->p, two, (uint64_t)ub, (const uint32_t *)m->d_tile.get(), t0, t1,
                                                            d_base, R.lower, R.upper, R.rows.get(), nrec, span, d_frag, d_nfrag,
                                                            (uint64_t)frag_cap, seq_base, row0_off))));
        HIP_TRY(hipGetLastError());
        if (!R.want_missing) continue;
        HIP_TRY(hipMemcpyAsync(h_nfrag, d_nfrag, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        const uint64_t nf = *h_nfrag;
        if (nf > frag_cap) { g_last_error = "sequence query: more fragments than a tile can emit"; return TSX_HIP_EHIP; }
        R.frag_h.resize(nf);
        if (nf) HIP_TRY(hipMemcpy(R.frag_h.data(), R.frag.get(), nf * sizeof(tsx_hip_seq_interval), hipMemcpyDeviceToHost));
        seq_merge_fragments(R);
    }
    hipLaunchKernelGGL(seq_finalize_kernel, dim3(grid_for(m, nrec, 8)), dim3(NT), 0, st, R.rows.get(), span, nrec, (uint64_t)nb_in);
    HIP_TRY(hipGetLastError());
    R.rows_h.resize(nrec);
    HIP_TRY(hipMemcpyAsync(R.rows_h.data(), R.rows.get(), nrec * sizeof(tsx_hip_seq_stats), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (R.window) TSX_TRY(track_merge(R, nrec, q_in != 0, nb_in, row0_off));
    size_t j = 0;
    if (q_in) {   // record 0 goes on with the open sequence
        tsx_hip_seq_stats &a = S.back();
        const tsx_hip_seq_stats &b = R.rows_h[0];
        if (b.kmers) a.min_count = a.kmers ? std::min(a.min_count, b.min_count) : b.min_count;
        a.length += b.length; a.kmers += b.kmers; a.present += b.present; a.sum_count += b.sum_count;
        j = 1;
    }
    for (size_t i = 0; j < nrec; ++j, ++i) {
        S.push_back(R.rows_h[j]);
        R.res->names += R.new_names[i];
        R.res->name_off.push_back(R.res->names.size());
    }
    return TSX_HIP_OK;
}

// What every sequence call does first; *res is set when it returns TSX_HIP_OK.
static int seq_begin(tsx_hip_map *m, uint64_t lower, uint64_t upper, tsx_hip_seq_result **res, hipStream_t st) {
    HIP_TRY(hipSetDevice(m->device));
    TSX_TRY(base_rule_ok(m));
    TSX_TRY(ensure_zeroed(m, st));
    TSX_TRY(fasta_begin(m, st));
    *res = new (std::nothrow) tsx_hip_seq_result();
    return *res ? TSX_HIP_OK : TSX_HIP_ENOMEM;
}
static int seq_end(int rc, tsx_hip_seq_result **res) {
    if (rc != TSX_HIP_OK) { delete *res; *res = nullptr; }
    return rc;
}

static int seq_host(tsx_hip_map *m, const char *text, size_t n, uint64_t lower, uint64_t upper, size_t chunk_bytes, bool missing,
                    uint64_t window, tsx_hip_seq_result **res) {
    if (!res) return TSX_HIP_EINVAL;
    *res = nullptr;
    if (int rca = seq_args_ok(m, lower, upper)) return rca;
    if (!text && n) return TSX_HIP_EINVAL;
    hipStream_t st = m->stream.get();
    join_foreign(m, false);
    TSX_TRY(seq_begin(m, lower, upper, res, st));
    if (!chunk_bytes) chunk_bytes = QUERY_CHUNK_DEFAULT;
    if (m->piece_fixed) chunk_bytes = std::min(chunk_bytes, m->piece);
    chunk_bytes = std::min(chunk_bytes, FA_PIECE_MAX);
    FastaScope fs(m);
    SeqRun R(m, st, lower, upper, missing, window, *res);
    int rc = R.init();
    // pieces are cut anywhere and overlap nowhere: what a sequence across the cut needs travels in the carries
    for (size_t off = 0; off < n && rc == TSX_HIP_OK; off += chunk_bytes) {
        const size_t len = std::min(chunk_bytes, n - off);
        rc = piece_upload(R.p, text + off, len);
        if (rc == TSX_HIP_OK) rc = seq_piece(R, R.p.text.get(), len);
    }
    return seq_end(rc, res);
}

static int seq_bgzf(tsx_hip_map *m, const void *gz, size_t n, uint64_t lower, uint64_t upper, bool missing, uint64_t window,
                    tsx_hip_seq_result **res) {
    if (!res) return TSX_HIP_EINVAL;
    *res = nullptr;
    if (int rca = seq_args_ok(m, lower, upper)) return rca;
    if (!gz && n) return TSX_HIP_EINVAL;
    BgzfIndex ix;
    if (!bgzf_index((const uint8_t *)gz, n, ix)) { g_last_error = "not a BGZF file (no BC extra field in every gzip member)"; return TSX_HIP_EINVAL; }
    hipStream_t st = m->stream.get();
    join_foreign(m, false);
    TSX_TRY(seq_begin(m, lower, upper, res, st));
    FastaScope fs(m);
    BgzfBatches bt(ix, std::min(bgzf_batch_bytes(), FA_PIECE_MAX));
    BgzfDev dv;
    DevBuf<uint8_t> txt;
    SeqRun R(m, st, lower, upper, missing, window, *res);   // (behind txt: its PieceBufs waits for the stream first)
    int rc = R.init();
    if (rc == TSX_HIP_OK && txt.alloc(bt.biggest() + 256) != TSX_HIP_OK) { g_last_error = "hipMalloc of a BGZF text buffer failed"; rc = TSX_HIP_ENOMEM; }
    for (; rc == TSX_HIP_OK && !bt.done(); bt.next()) {
        rc = inflate_batch((const uint8_t *)gz, n, ix, bt.m0, bt.m1, dv, txt.get(), st);
        if (rc == TSX_HIP_OK) rc = seq_piece(R, txt.get(), bt.text());
    }
    (void)hipStreamSynchronize(st);   // nothing queued may outlive dv
    return seq_end(rc, res);
}

static int seq_device(tsx_hip_map *m, const void *dev_text, size_t n, uint64_t lower, uint64_t upper, bool missing,
                      uint64_t window, tsx_hip_seq_result **res, void *stream) {
    if (!res) return TSX_HIP_EINVAL;
    *res = nullptr;
    if (int rca = seq_args_ok(m, lower, upper)) return rca;
    if ((!dev_text && n) || ((uintptr_t)dev_text & 15)) return TSX_HIP_EINVAL;
    hipStream_t st = pick_stream(m, stream);
    TSX_TRY(seq_begin(m, lower, upper, res, st));
    FastaScope fs(m);
    SeqRun R(m, st, lower, upper, missing, window, *res);
    int rc = R.init();
    const uint8_t *base = (const uint8_t *)dev_text;
    const size_t WIN = std::min(dev_window_bytes(), FA_PIECE_MAX);
    for (size_t off = 0; off < n && rc == TSX_HIP_OK; off += WIN) rc = seq_piece(R, base + off, std::min(WIN, n - off));
    return seq_end(rc, res);
}

extern "C" int tsx_hip_seq_stats_host(tsx_hip_map *m, const char *text, size_t n, uint64_t lower, uint64_t upper, size_t chunk_bytes,
                                      tsx_hip_seq_result **res) {
    return seq_host(m, text, n, lower, upper, chunk_bytes, false, 0, res);
}
extern "C" int tsx_hip_seq_missing_host(tsx_hip_map *m, const char *text, size_t n, uint64_t lower, uint64_t upper, size_t chunk_bytes,
                                        tsx_hip_seq_result **res) {
    return seq_host(m, text, n, lower, upper, chunk_bytes, true, 0, res);
}
extern "C" int tsx_hip_seq_stats_bgzf_host(tsx_hip_map *m, const void *gz, size_t n, uint64_t lower, uint64_t upper,
                                           tsx_hip_seq_result **res) {
    return seq_bgzf(m, gz, n, lower, upper, false, 0, res);
}
extern "C" int tsx_hip_seq_missing_bgzf_host(tsx_hip_map *m, const void *gz, size_t n, uint64_t lower, uint64_t upper,
                                             tsx_hip_seq_result **res) {
    return seq_bgzf(m, gz, n, lower, upper, true, 0, res);
}
extern "C" int tsx_hip_seq_stats_device(tsx_hip_map *m, const void *dev_text, size_t n, uint64_t lower, uint64_t upper,
                                        tsx_hip_seq_result **res, void *stream) {
    return seq_device(m, dev_text, n, lower, upper, false, 0, res, stream);
}
extern "C" int tsx_hip_seq_missing_device(tsx_hip_map *m, const void *dev_text, size_t n, uint64_t lower, uint64_t upper,
                                          tsx_hip_seq_result **res, void *stream) {
    return seq_device(m, dev_text, n, lower, upper, true, 0, res, stream);
}

// The track calls: what the stats calls refuse first, then the window.
static int track_args_ok(const tsx_hip_map *m, uint64_t lower, uint64_t upper, uint64_t window) {
    if (int rca = seq_args_ok(m, lower, upper)) return rca;
    if (window < 64 || window > ((uint64_t)1 << 32)) return seq_fail("sequence track: window outside 64 .. 2^32");
    return TSX_HIP_OK;
}
extern "C" int tsx_hip_seq_track_host(tsx_hip_map *m, const char *text, size_t n, uint64_t lower, uint64_t upper, uint64_t window,
                                      size_t chunk_bytes, tsx_hip_seq_result **res) {
    if (res) *res = nullptr;
    if (int rca = track_args_ok(m, lower, upper, window)) return rca;
    return seq_host(m, text, n, lower, upper, chunk_bytes, false, window, res);
}
extern "C" int tsx_hip_seq_track_bgzf_host(tsx_hip_map *m, const void *gz, size_t n, uint64_t lower, uint64_t upper, uint64_t window,
                                           tsx_hip_seq_result **res) {
    if (res) *res = nullptr;
    if (int rca = track_args_ok(m, lower, upper, window)) return rca;
    return seq_bgzf(m, gz, n, lower, upper, false, window, res);
}
extern "C" int tsx_hip_seq_track_device(tsx_hip_map *m, const void *dev_text, size_t n, uint64_t lower, uint64_t upper, uint64_t window,
                                        tsx_hip_seq_result **res, void *stream) {
    if (res) *res = nullptr;
    if (int rca = track_args_ok(m, lower, upper, window)) return rca;
    return seq_device(m, dev_text, n, lower, upper, false, window, res, stream);
}
extern "C" size_t tsx_hip_seq_result_bins(const tsx_hip_seq_result *res, const tsx_hip_seq_bin **bins, const uint64_t **first) {
    const bool track = res && res->window;   // (a result without a track keeps no offsets)
    if (bins) *bins = track ? res->bins.data() : nullptr;
    if (first) *first = track ? res->first.data() : nullptr;
    return track ? res->bins.size() : 0;
}
extern "C" uint64_t tsx_hip_seq_result_window(const tsx_hip_seq_result *res) { return res ? res->window : 0; }

extern "C" size_t tsx_hip_seq_result_count(const tsx_hip_seq_result *res) { return res ? res->stats.size() : 0; }
extern "C" const tsx_hip_seq_stats *tsx_hip_seq_result_stats(const tsx_hip_seq_result *res) { return res ? res->stats.data() : nullptr; }
extern "C" const char *tsx_hip_seq_result_names(const tsx_hip_seq_result *res, const uint64_t **offsets) {
    if (offsets) *offsets = res ? res->name_off.data() : nullptr;
    return res ? res->names.data() : nullptr;
}
extern "C" size_t tsx_hip_seq_result_intervals(const tsx_hip_seq_result *res, const tsx_hip_seq_interval **intervals) {
    if (intervals) *intervals = res ? res->iv.data() : nullptr;
    return res ? res->iv.size() : 0;
}
extern "C" void tsx_hip_seq_result_free(tsx_hip_seq_result *res) { delete res; }

// "inf" when nothing is missing, "NA" without k-mers, else -10 log10(1 - (present / kmers)^(1 / k)) as %.4f (-0 as 0).
static void seq_qv_text(uint64_t present, uint64_t kmers, int k, char (&out)[32]) {
    if (kmers == 0) { snprintf(out, sizeof out, "NA"); return; }
    if (present == kmers) { snprintf(out, sizeof out, "inf"); return; }
    double v = -10.0 * log10(1.0 - pow((double)present / (double)kmers, 1.0 / (double)k));
    if (!(v > 0.0)) v = 0.0;
    snprintf(out, sizeof out, "%.4f", v);
}
static void seq_name_text(const tsx_hip_seq_result *res, size_t i, std::string &out) {
    const size_t a = (size_t)res->name_off[i], b = (size_t)res->name_off[i + 1];
    if (a == b) out += '*';
    else out.append(res->names, a, b - a);
}

extern "C" int tsx_hip_seq_write_stats(const tsx_hip_seq_result *res, int k, int fd) {
    if (!res || k < 1 || fd < 0) return TSX_HIP_EINVAL;
    std::string out;
    char num[160], qv[32];
    for (size_t i = 0; i < res->stats.size(); ++i) {
        const tsx_hip_seq_stats &s = res->stats[i];
        seq_name_text(res, i, out);
        seq_qv_text(s.present, s.kmers, k, qv);
        snprintf(num, sizeof num, "\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%s\n", (unsigned long long)s.length, (unsigned long long)s.kmers,
                 (unsigned long long)s.present, (unsigned long long)(s.kmers - s.present), (unsigned long long)s.min_count,
                 (unsigned long long)s.sum_count, qv);
        out += num;
        if (out.size() >= ((size_t)1 << 20)) { TSX_TRY(write_all(fd, (const uint8_t *)out.data(), out.size())); out.clear(); }
    }
    return write_all(fd, (const uint8_t *)out.data(), out.size());
}

extern "C" int tsx_hip_seq_write_missing(const tsx_hip_seq_result *res, int fd) {
    if (!res || fd < 0) return TSX_HIP_EINVAL;
    std::string out;
    char num[64];
    for (const tsx_hip_seq_interval &v : res->iv) {
        if (v.seq >= res->stats.size()) return TSX_HIP_EINVAL;
        seq_name_text(res, (size_t)v.seq, out);
        snprintf(num, sizeof num, "\t%llu\t%llu\n", (unsigned long long)v.start, (unsigned long long)v.end);
        out += num;
        if (out.size() >= ((size_t)1 << 20)) { TSX_TRY(write_all(fd, (const uint8_t *)out.data(), out.size())); out.clear(); }
    }
    return write_all(fd, (const uint8_t *)out.data(), out.size());
}

extern "C" int tsx_hip_seq_write_track(const tsx_hip_seq_result *res, int fd) {
    if (!res || fd < 0) return TSX_HIP_EINVAL;
    if (!res->window) return seq_fail("sequence track: the result holds no track");
    std::string out;
    char num[200], mean[40];
    const uint64_t W = res->window;
    for (size_t i = 0; i < res->stats.size(); ++i) {
        const uint64_t L = res->stats[i].length;
        for (uint64_t b = 0, at = res->first[i]; at < res->first[i + 1]; ++b, ++at) {
            const tsx_hip_seq_bin &v = res->bins[(size_t)at];
            if (v.kmers) snprintf(mean, sizeof mean, "%.4f", (double)v.sum_count / (double)v.kmers);
            else snprintf(mean, sizeof mean, "NA");
            seq_name_text(res, i, out);
            snprintf(num, sizeof num, "\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%s\n", (unsigned long long)(b * W),
                     (unsigned long long)std::min((b + 1) * W, L), (unsigned long long)v.kmers, (unsigned long long)v.present,
                     (unsigned long long)v.min_count, (unsigned long long)v.max_count, mean);
            out += num;
            if (out.size() >= ((size_t)1 << 20)) { TSX_TRY(write_all(fd, (const uint8_t *)out.data(), out.size())); out.clear(); }
        }
    }
    return write_all(fd, (const uint8_t *)out.data(), out.size());
}

// ---- read binning by two tables: hits in A and in B per record, one output per class (tsx_bin.h) ------------------
static int bin_fail(const char *why) { g_last_error = why; return TSX_HIP_EINVAL; }

// What the bin calls refuse, before any device call: the rule first, then the tables (the conditions of tsx_hip_combine).
static int bin_rule_check(const tsx_hip_bin_rule *r) {
    if (!r) return bin_fail("bin: no rule");
    if (std::max<uint64_t>(1, r->a_lower) > r->a_upper) return bin_fail("bin: a_lower > a_upper");
    if (std::max<uint64_t>(1, r->b_lower) > r->b_upper) return bin_fail("bin: b_lower > b_upper");
    if (r->ratio_milli < 1000u || r->ratio_milli > 1000000u) return bin_fail("bin: ratio_milli outside 1000 .. 1000000");
    if (r->reserved != 0) return bin_fail("bin: reserved is not 0");
    return TSX_HIP_OK;
}
static int bin_check(const tsx_hip_map *a, const tsx_hip_map *b, const tsx_hip_bin_rule *r) {
    TSX_TRY(bin_rule_check(r));
    if (!a || !b) return bin_fail("bin: a and b are needed");
    if (a->p.lg != a->p.l || b->p.lg != b->p.l) return bin_fail("bin: a shard of a multi-GPU table");
    if (b->device != a->device) return bin_fail("bin: the tables are on different devices");
    if (b->p.k != a->p.k) return bin_fail("bin: the tables differ in k");
    if (b->canon != a->canon) return bin_fail("bin: the tables differ in canonical mode");
    if (b->p.acgt_only != a->p.acgt_only || b->minq != a->minq) return bin_fail("bin: the tables differ in base rule");
    return base_rule_ok(a);
}
static int bin_io_check(const tsx_hip_bin_io *io) {
    if (!io) return bin_fail("bin: no outputs (io is NULL)");
    if (io->fd_a == -1 && io->fd_b == -1 && io->fd_ambiguous == -1 && io->fd_none == -1)
        return bin_fail("bin: every output of io is -1");
    return TSX_HIP_OK;
}

// Behind everything queued on the two maps (a caller's stream of an earlier call too); lazily cleared tables are zeroed
// before anyone reads them.  Both maps' streams are idle afterwards: B's has nothing left for A's to wait for.
static int bin_begin(tsx_hip_map *a, tsx_hip_map *b) {
    HIP_TRY(hipSetDevice(a->device));
    for (tsx_hip_map *m : {a, b}) {
        join_foreign(m, true);
        TSX_TRY(ensure_zeroed(m, m->stream.get()));
        if (m->join_ev.get()) {   // (B's stream in front of A's by an event, then the wait the contract asks for)
            HIP_TRY(hipEventRecord(m->join_ev.get(), m->stream.get()));
            HIP_TRY(hipStreamWaitEvent(a->stream.get(), m->join_ev.get(), 0));
        }
        HIP_TRY(hipStreamSynchronize(m->stream.get()));
    }
    return TSX_HIP_OK;
}

// bin_reads_kernel over the start positions [0, own_end) of d_text (n readable bytes), after line_pass on A's scratch.
// One LUT when A and B hash alike (the same seed makes the same mapping for one k).
static int bin_launch(tsx_hip_map *a, const tsx_hip_map *b, const uint8_t *d_text, uint64_t n, uint64_t own_end, int head_open,
                      const unsigned long long *d_line_base, const tsx_hip_bin_rule &r, unsigned long long *d_stats, uint64_t cap,
                      hipStream_t st) {
    if (own_end == 0) return TSX_HIP_OK;
    const uint64_t ntiles = (own_end + TILE - 1) / TILE;
    const bool one = a->seed == b->seed && a->lut == b->lut;
    const size_t lds = a->lut.size() * 8 * (one ? 1 : 2);
    const int grid = (int)std::min<uint64_t>(ntiles, (uint64_t)a->cus * 4);
    const uint32_t lshift = line_shift(a);
    const BinRanges rg = {std::max<uint64_t>(1, r.a_lower), r.a_upper, std::max<uint64_t>(1, r.b_lower), r.b_upper};
    hipError_t attr = hipSuccess;
#define TSX_BIN(FORMV)                                                                                                       \
    {                                                                                                                        \
        auto kern = (bin_reads_kernel<WKV, CANV, BRV, FORMV>);                                                               \
        attr = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                \
        if (attr == hipSuccess)                                                                                              \
            hipLaunchKernelGGL(kern, dim3(grid), dim3(NT), lds, st, a->p, b->p, d_text, n, own_end, head_open,               \
                               (const uint32_t *)a->d_tile.get(), ntiles, d_line_base, lshift, rg, d_stats, cap, a->qmap_cur); \
    }
    if (one) { DISPATCH_BR(a, DISPATCH_CANON(a, DISPATCH_WK(a, TSX_BIN(BIN_ONE_LUT)))); }
    else { DISPATCH_BR(a, DISPATCH_CANON(a, DISPATCH_WK(a, TSX_BIN(BIN_TWO_LUT)))); }
#undef TSX_BIN
    HIP_TRY(attr);
    HIP_TRY(hipGetLastError());
    return TSX_HIP_OK;
}

extern "C" int tsx_hip_bin_stats_device(tsx_hip_map *a, tsx_hip_map *b, const void *dev_text, size_t n, const tsx_hip_bin_rule *rule,
                                        void *dev_stats, size_t stats_cap, size_t *n_records, void *stream) {
    if (n_records) *n_records = 0;
    TSX_TRY(bin_check(a, b, rule));
    if ((!dev_text && n) || ((uintptr_t)dev_text & 15) || (!dev_stats && stats_cap)) return bin_fail("bin: the text or the stats pointer");
    TSX_TRY(bin_begin(a, b));
    hipStream_t st = pick_stream(a, stream);
    const uint8_t *base = (const uint8_t *)dev_text;
    unsigned long long *stats = (unsigned long long *)dev_stats;
    if (stats_cap) HIP_TRY(hipMemsetAsync(stats, 0, stats_cap * sizeof(tsx_hip_bin_stats), st));
    TSX_TRY(device_windows(a, base, n, false, st,
                           [&](size_t off, size_t own, size_t len, int head_open, bool, const unsigned long long *d_base) {
                               return bin_launch(a, b, base + off, len, own, head_open, d_base, *rule, stats, stats_cap, st);
                           }));
    return windows_records(a, stats_cap, n_records, st);
}

// Scratch of one bin call that works on pieces.  words: the records of each class [0..4), the bytes of each output [4..8).
struct BinBufs {
    DevBuf<unsigned long long> stats;
    DevBuf<uint8_t> cls;
    DevBuf<unsigned long long> words;
    PinBuf<unsigned long long> h_words;
    Compaction out[4];   // one per class: its lengths and its bytes
    PieceBufs p;
    explicit BinBufs(hipStream_t s) : p(s) {}
    int init() {
        TSX_TRY(words.alloc(8 * sizeof(unsigned long long)));
        HIP_TRY(hipMemsetAsync(words.get(), 0, 8 * sizeof(unsigned long long), p.st));
        return h_words.alloc(8 * sizeof(unsigned long long));
    }
};

// One piece: piece_front, then -- when it holds a whole record -- the stats and the classes of its records [0, nrec),
// queued and not waited for.
static int bin_piece(tsx_hip_map *a, const tsx_hip_map *b, BinBufs &bb, const uint8_t *d_text, uint64_t len, bool last,
                     const tsx_hip_bin_rule &r, bool spans, hipStream_t st, uint64_t &cut, uint64_t &nrec, bool &open) {
    TSX_TRY(piece_front(a, bb.p, d_text, len, last, spans, cut, nrec, open));
    if (nrec == 0) return TSX_HIP_OK;
    TSX_TRY(grow(st, bb.stats, nrec * sizeof(tsx_hip_bin_stats)));
    TSX_TRY(grow(st, bb.cls, nrec));
    HIP_TRY(hipMemsetAsync(bb.stats.get(), 0, nrec * sizeof(tsx_hip_bin_stats), st));
    QmapScope qs(a);
    TSX_TRY(piece_qmap(a, d_text, cut, st));
    TSX_TRY(bin_launch(a, b, d_text, cut, cut, 0, bb.p.info.get() + 4, r, bb.stats.get(), nrec, st));
    hipLaunchKernelGGL(bin_class_kernel, dim3(grid_for(a, nrec, 8)), dim3(NT), 0, st, (const unsigned long long *)bb.stats.get(),
                       nrec, r.min_hits, r.ratio_milli, bb.cls.get(), bb.words.get());
    HIP_TRY(hipGetLastError());
    return TSX_HIP_OK;
}

// Stats (io == NULL: each piece's stats and classes go to the caller's arrays while they fit) and binned reads (one
// write-behind per wanted output: piece i + 1 is scanned and compacted while piece i's outputs are written).
static int bin_host(tsx_hip_map *a, tsx_hip_map *b, const char *text, size_t n, const tsx_hip_bin_rule &r, size_t chunk_bytes,
                    tsx_hip_bin_stats *stats_out, uint8_t *class_out, size_t stats_cap, size_t *n_records,
                    const tsx_hip_bin_io *io, tsx_hip_bin_totals *totals) {
    TSX_TRY(bin_begin(a, b));
    hipStream_t st = a->stream.get();
    WriteBehind wb[4];
    if (io) { wb[0].fd = io->fd_a; wb[1].fd = io->fd_b; wb[2].fd = io->fd_ambiguous; wb[3].fd = io->fd_none; }
    BinBufs bb(st);
    tsx_hip_bin_totals t;
    memset(&t, 0, sizeof t);
    uint64_t rec_base = 0;
    int rc = bb.init();
    if (rc == TSX_HIP_OK) rc = host_pieces(a, bb.p, text, n, chunk_bytes, false, rec_base,
        [&](const uint8_t *d_text, uint64_t len, bool last, uint64_t &cut, uint64_t &nrec, bool &open) {
            return bin_piece(a, b, bb, d_text, len, last, r, io != nullptr, st, cut, nrec, open);
        },
        [&](size_t, uint64_t base, uint64_t cut, uint64_t nrec, bool open) -> int {
            if (!io) {
                TSX_TRY(deliver_records(stats_out, stats_cap, base, bb.stats.get(), nrec, st));
                return class_out ? deliver_records(class_out, stats_cap, base, bb.cls.get(), nrec, st) : TSX_HIP_OK;
            }
            if (!nrec) return TSX_HIP_OK;
            unsigned long long *const words = bb.words.get();
            const unsigned long long *h = bb.h_words.get();
            const uint8_t *d_out[4] = {nullptr, nullptr, nullptr, nullptr};
            const uint64_t cuts[4] = {cut, cut, cut, cut};
            for (uint32_t c = 0; c < 4; ++c) {   // the existing scan and copy kernels, once per wanted output
                if (wb[c].fd < 0) continue;
                unsigned long long *len;
                TSX_TRY(bb.out[c].lengths(st, nrec, len));
                hipLaunchKernelGGL(bin_len_kernel, dim3(grid_for(a, nrec, 8)), dim3(NT), 0, st, (const uint8_t *)bb.cls.get(),
                                   (const unsigned long long *)bb.p.rspan.get(), nrec, c, open ? 1 : 0, len);
                TSX_TRY(bb.out[c].copy_spans(a, bb.p.text.get(), cut, bb.p.rspan.get(), nrec, words + 4 + c, st));
                d_out[c] = bb.out[c].out.out;
            }
            TSX_TRY(WriteBehind::words_back(wb, 4, words, bb.h_words.get(), 8, bb.p.ev.get(), st));
            for (uint32_t c = 0; c < 4; ++c) t.n[c] += h[c];
            return WriteBehind::stage_all(wb, 4, d_out, h + 4, cuts, "bin", words, 8, st);
        });
    for (WriteBehind &w : wb)
        if (rc == TSX_HIP_OK) rc = w.flush();
    if (n_records) *n_records = (size_t)rec_base;
    t.records = rec_base;
    for (int c = 0; c < 4; ++c) t.bytes[c] = wb[c].bytes;
    if (totals) *totals = t;
    if (rc == TSX_HIP_OK && !io && rec_base > stats_cap) rc = TSX_HIP_ERANGE;
    return rc;
}

extern "C" int tsx_hip_bin_stats_host(tsx_hip_map *a, tsx_hip_map *b, const char *text, size_t n, const tsx_hip_bin_rule *rule,
                                      tsx_hip_bin_stats *stats_out, uint8_t *class_out, size_t stats_cap, size_t *n_records,
                                      size_t chunk_bytes) {
    if (n_records) *n_records = 0;
    TSX_TRY(bin_check(a, b, rule));
    if ((!text && n) || (!stats_out && stats_cap)) return bin_fail("bin: the text or the stats pointer");
    return bin_host(a, b, text, n, *rule, chunk_bytes, stats_out, class_out, stats_cap, n_records, nullptr, nullptr);
}

extern "C" int tsx_hip_bin_reads_host(tsx_hip_map *a, tsx_hip_map *b, const char *text, size_t n, const tsx_hip_bin_rule *rule,
                                      const tsx_hip_bin_io *io, size_t chunk_bytes, tsx_hip_bin_totals *totals) {
    if (totals) memset(totals, 0, sizeof *totals);
    TSX_TRY(bin_rule_check(rule));
    TSX_TRY(bin_io_check(io));
    TSX_TRY(bin_check(a, b, rule));
    if (!text && n) return bin_fail("bin: no text");
    return bin_host(a, b, text, n, *rule, chunk_bytes, nullptr, nullptr, 0, nullptr, io, totals);
}

// ---- read trimming: the solid stretch of every record (tsx_trim.h) ------------------------------------------------
static bool trim_rule_ok(const tsx_hip_map *m, const tsx_hip_trim_rule *r) {
    return r && query_args_ok(m, r->lower, r->upper) && (r->mode == TSX_HIP_TRIM_LONGEST || r->mode == TSX_HIP_TRIM_PREFIX) &&
           r->reserved == 0;
}

// solid_bits_kernel over the start positions [0, own_end) of d_text (n readable bytes), after line_pass.
static int solid_launch(tsx_hip_map *m, const uint8_t *d_text, uint64_t n, uint64_t own_end, int head_open,
                        const unsigned long long *d_line_base, const tsx_hip_trim_rule &rule, unsigned long long *d_bits,
                        hipStream_t st) {
    if (own_end == 0) return TSX_HIP_OK;
    const uint64_t ntiles = (own_end + TILE - 1) / TILE;
    const size_t lut_bytes = m->lut.size() * 8;
    const int grid = (int)std::min<uint64_t>(ntiles, (uint64_t)m->cus * 4);
    DISPATCH_BR(m, DISPATCH_CANON(m, DISPATCH_WK(m, hipLaunchKernelGGL((solid_bits_kernel<WKV, CANV, BRV>), dim3(grid), dim3(NT),
                                                        lut_bytes, st, m->p, d_text, n, own_end, head_open,
                                                        (const uint32_t *)m->d_tile.get(), ntiles, d_line_base, rule.lower,
                                                        rule.upper, d_bits, m->qmap_cur))));
    HIP_TRY(hipGetLastError());
    return TSX_HIP_OK;
}

// trim_lines_kernel over the start positions [0, own_end) of d_text (n readable bytes, `off` into its whole text), after
// line_pass: the line offsets of the records < cap in lo.  `last`: the text ends here, and d_carry holds the line
// ends up to there (an unterminated last line).
static void lines_launch(tsx_hip_map *m, const uint8_t *d_text, uint64_t n, uint64_t own_end, int head_open,
                         const unsigned long long *d_line_base, uint64_t off, bool last, unsigned long long *lo, uint64_t cap,
                         hipStream_t st) {
    const uint64_t ntiles = (own_end + TILE - 1) / TILE;
    const uint32_t lshift = line_shift(m);
    hipLaunchKernelGGL(trim_lines_kernel, dim3((uint32_t)std::min<uint64_t>(ntiles, (uint64_t)m->cus * 8)), dim3(NT), 0, st,
                       d_text, n, own_end, head_open, (const uint32_t *)m->d_tile.get(), ntiles, d_line_base,
                       (const uint32_t *)m->d_carry.get(), lshift, off, last ? 1 : 0, lo, cap);
}

// Spans of a device text in windows (device_windows): every window adds its words to one bitmap of the whole text and
// its line offsets to one array; the runs are walked once, after the last window.
extern "C" int tsx_hip_trim_spans_device(tsx_hip_map *m, const void *dev_text, size_t n, const tsx_hip_trim_rule *rule,
                                         void *dev_spans, size_t spans_cap, size_t *n_records, void *stream) {
    if (n_records) *n_records = 0;
    if (!trim_rule_ok(m, rule) || (!dev_text && n) || ((uintptr_t)dev_text & 15) || (!dev_spans && spans_cap)) return TSX_HIP_EINVAL;
    hipStream_t st;
    TSX_TRY(device_begin(m, stream, st));
    const uint64_t cap = std::min<uint64_t>(spans_cap, max_records(m, n)), nwords = ((uint64_t)n + 63) / 64;
    DevBuf<unsigned long long> bits, lo;
    SyncAtExit wait(st);
    TSX_TRY(bits.alloc((nwords + 1) * 8));
    TSX_TRY(lo.alloc((cap + 1) * TL_N * 8));
    const uint8_t *base = (const uint8_t *)dev_text;
    unsigned long long *span = (unsigned long long *)dev_spans;
    if (spans_cap) HIP_TRY(hipMemsetAsync(span, 0, spans_cap * sizeof(tsx_hip_trim_span), st));
    HIP_TRY(hipMemsetAsync(lo.get(), 0, (cap + 1) * TL_N * 8, st));
    TSX_TRY(device_windows(m, base, n, true, st,   // (whole bitmap words)
                           [&](size_t off, size_t own, size_t len, int head_open, bool last, const unsigned long long *d_base) -> int {
                               TSX_TRY(solid_launch(m, base + off, len, own, head_open, d_base, *rule, bits.get() + off / 64, st));
                               lines_launch(m, base + off, len, own, head_open, d_base, off, last, lo.get(), cap, st);
                               return TSX_HIP_OK;
                           }));
    if (cap && nwords) {
        const unsigned long long *d_nrec = (const unsigned long long *)m->d_carry.get() + 3;
        hipLaunchKernelGGL(trim_run_kernel, dim3(grid_for(m, nwords, 8)), dim3(NT), 0, st, (const unsigned long long *)bits.get(),
                           nwords, (const unsigned long long *)lo.get(), d_nrec, (uint64_t)0, cap, (uint32_t)m->p.k, (int)rule->mode,
                           span);
        hipLaunchKernelGGL(trim_finalize_kernel, dim3(grid_for(m, cap, 8)), dim3(NT), 0, st, span, cap, d_nrec, (uint64_t)0);
    }
    return windows_records(m, spans_cap, n_records, st);
}

// Scratch of one trim call that works on pieces.
struct TrimBufs {
    DevBuf<unsigned long long> bits, lo, span, src;   // (span: the packed runs, then the spans; src: where a segment starts)
    Compaction c;      // the segment lengths and the trimmed records
    PieceBufs p;
    explicit TrimBufs(hipStream_t s) : p(s) {}
};

// The records [0, nrec) of d_text[0, cut), after a line pass over a text that starts with [0, cut): bitmap, line offsets
// and runs (b.span holds the packed runs).  `last`: [0, cut) ends the text, and d_carry holds its line ends (an
// unterminated last line).  Queued, not waited for.
static int trim_records(tsx_hip_map *m, TrimBufs &b, const uint8_t *d_text, uint64_t cut, uint64_t nrec, bool last,
                        const tsx_hip_trim_rule &rule, hipStream_t st) {
    const uint64_t nwords = (cut + 63) / 64;
    TSX_TRY(grow(st, b.bits, (nwords + 1) * 8));
    TSX_TRY(grow(st, b.lo, nrec * TL_N * 8));
    TSX_TRY(grow(st, b.span, nrec * sizeof(tsx_hip_trim_span)));
    HIP_TRY(hipMemsetAsync(b.lo.get(), 0, nrec * TL_N * 8, st));
    HIP_TRY(hipMemsetAsync(b.span.get(), 0, nrec * sizeof(tsx_hip_trim_span), st));
    QmapScope qs(m);
    TSX_TRY(piece_qmap(m, d_text, cut, st));
    const unsigned long long *zero = b.p.info.get() + 4;
    TSX_TRY(solid_launch(m, d_text, cut, cut, 0, zero, rule, b.bits.get(), st));
    // (the carry is read for an unterminated last line only: then cut = len and it holds the lines of [0, cut))
    lines_launch(m, d_text, cut, cut, 0, zero, 0, last, b.lo.get(), nrec, st);
    hipLaunchKernelGGL(trim_run_kernel, dim3(grid_for(m, nwords, 8)), dim3(NT), 0, st, (const unsigned long long *)b.bits.get(),
                       nwords, (const unsigned long long *)b.lo.get(), (const unsigned long long *)nullptr, nrec, nrec,
                       (uint32_t)m->p.k, (int)rule.mode, b.span.get());
    HIP_TRY(hipGetLastError());
    return TSX_HIP_OK;
}

// Behind trim_records: the four segment lengths of every record in b.c (4 nrec + 1 entries, the last 0), their sources
// in b.src, tot[0..2] += records written, bases in, bases kept.
static int trim_lens(tsx_hip_map *m, TrimBufs &b, uint64_t nrec, const tsx_hip_trim_rule &rule, unsigned long long *tot,
                     hipStream_t st) {
    const uint32_t lpr = m->p.line_mask + 1;
    unsigned long long *seg;
    TSX_TRY(b.c.lengths(st, nrec * 4, seg));
    TSX_TRY(grow(st, b.src, nrec * 4 * sizeof(unsigned long long)));
    hipLaunchKernelGGL(trim_len_kernel, dim3(grid_for(m, nrec, 8)), dim3(NT), 0, st, b.span.get(),
                       (const unsigned long long *)b.lo.get(), nrec, lpr, rule.min_len ? rule.min_len : (uint64_t)m->p.k, seg,
                       b.src.get(), tot);
    HIP_TRY(hipGetLastError());
    return TSX_HIP_OK;
}

// One piece: piece_front, then over its whole records [0, cut): bitmap, line offsets, runs, and either the spans alone
// (b.span, finalized) or -- `copy` -- the segment lengths, their scan (total -> info[3], totals -> info[5..7]) and the
// output in b.c.out.  What follows the wait is queued, not waited for.  Not last and no whole record: nrec = 0, nothing
// done.
static int trim_piece(tsx_hip_map *m, TrimBufs &b, const uint8_t *d_text, uint64_t len, bool last,
                      const tsx_hip_trim_rule &rule, bool copy, hipStream_t st, uint64_t &cut, uint64_t &nrec) {
    bool open;
    TSX_TRY(piece_front(m, b.p, d_text, len, last, false, cut, nrec, open));
    if (nrec == 0) return TSX_HIP_OK;
    TSX_TRY(trim_records(m, b, d_text, cut, nrec, last, rule, st));
    if (!copy) {
        hipLaunchKernelGGL(trim_finalize_kernel, dim3(grid_for(m, nrec, 8)), dim3(NT), 0, st, b.span.get(), nrec,
                           (const unsigned long long *)nullptr, nrec);
        HIP_TRY(hipGetLastError());
        return TSX_HIP_OK;
    }
    TSX_TRY(trim_lens(m, b, nrec, rule, b.p.info.get() + 5, st));
    return b.c.copy_segments(m, d_text, cut, b.src.get(), nrec * 4, b.p.info.get() + 3, st);
}

// Spans and trimmed reads: the pieces of host_pieces.  fd < 0: each piece's spans go to spans_out[rec_base ..] while
// they fit.  Else write-behind to fd.
static int trim_host(tsx_hip_map *m, const char *text, size_t n, const tsx_hip_trim_rule &rule, size_t chunk_bytes,
                     tsx_hip_trim_span *spans_out, size_t spans_cap, size_t *n_records, int fd, tsx_hip_trim_totals *totals) {
    hipStream_t st = m->stream.get();
    WriteBehind wb;
    wb.fd = fd;
    TrimBufs b(st);
    uint64_t records = 0, tot[3] = {0, 0, 0};   // kept, bases in, bases kept
    int rc = host_pieces(m, b.p, text, n, chunk_bytes, false, records,
        [&](const uint8_t *d_text, uint64_t len, bool last, uint64_t &cut, uint64_t &nrec, bool &) {
            return trim_piece(m, b, d_text, len, last, rule, fd >= 0, st, cut, nrec);
        },
        [&](size_t, uint64_t base, uint64_t cut, uint64_t nrec, bool) -> int {
            if (fd < 0) return deliver_records(spans_out, spans_cap, base, b.span.get(), nrec, st);
            return nrec ? wb.piece(b.p, b.c.out.out, cut, 3, tot, "trim") : TSX_HIP_OK;
        });
    if (rc == TSX_HIP_OK) rc = wb.flush();
    if (n_records) *n_records = (size_t)records;
    if (totals) *totals = tsx_hip_trim_totals{records, tot[0], tot[1], tot[2], wb.bytes};
    if (rc == TSX_HIP_OK && fd < 0 && records > spans_cap) rc = TSX_HIP_ERANGE;
    return rc;
}

extern "C" int tsx_hip_trim_spans_host(tsx_hip_map *m, const char *text, size_t n, const tsx_hip_trim_rule *rule,
                                       tsx_hip_trim_span *spans_out, size_t spans_cap, size_t *n_records, size_t chunk_bytes) {
    if (n_records) *n_records = 0;
    if (!trim_rule_ok(m, rule) || (!text && n) || (!spans_out && spans_cap)) return TSX_HIP_EINVAL;
    return trim_host(m, text, n, *rule, chunk_bytes, spans_out, spans_cap, n_records, -1, nullptr);
}

extern "C" int tsx_hip_trim_reads_host(tsx_hip_map *m, const char *text, size_t n, const tsx_hip_trim_rule *rule, int fd,
                                       size_t chunk_bytes, tsx_hip_trim_totals *totals) {
    if (totals) *totals = tsx_hip_trim_totals{0, 0, 0, 0, 0};
    if (!trim_rule_ok(m, rule) || (!text && n) || fd < 0) return TSX_HIP_EINVAL;
    return trim_host(m, text, n, *rule, chunk_bytes, nullptr, 0, nullptr, fd, totals);
}

extern "C" int tsx_hip_trim_reads_device(tsx_hip_map *m, const void *dev_text, size_t n, const tsx_hip_trim_rule *rule,
                                         void *dev_out, size_t out_cap, tsx_hip_trim_totals *totals, void *stream) {
    if (totals) *totals = tsx_hip_trim_totals{0, 0, 0, 0, 0};
    if (!trim_rule_ok(m, rule) || (!dev_text && n) || ((uintptr_t)dev_text & 15) || !dev_out || ((uintptr_t)dev_out & 15) ||
        n >= QUERY_PIECE_MAX)
        return TSX_HIP_EINVAL;
    if (out_cap < n + 64) return TSX_HIP_ERANGE;
    hipStream_t st;
    TSX_TRY(device_begin(m, stream, st));
    TrimBufs b(st);
    int rc = b.p.init();
    b.c.out.out = (uint8_t *)dev_out; b.c.out.have = out_cap;   // the copy writes the caller's buffer (never grown)
    uint64_t cut = 0, nrec = 0;
    const unsigned long long *h = nullptr;
    if (rc == TSX_HIP_OK) rc = trim_piece(m, b, (const uint8_t *)dev_text, n, true, *rule, true, st, cut, nrec);
    if (rc == TSX_HIP_OK && nrec) rc = piece_words(b.p, 5, cut, "trim", h);
    if (totals && h) *totals = tsx_hip_trim_totals{nrec, h[5], h[6], h[7], h[3]};
    return rc;
}

// ---- read correction: single substitutions undone from the spectrum (tsx_correct.h) ----------------------------------
static_assert(sizeof(tsx_hip_correction) == sizeof(CorrectionRec) && sizeof(tsx_hip_correct_totals) == 48 &&
                  sizeof(tsx_hip_correct_rule) == 24, "the correction records of the ABI are the kernels'");
static int correct_fail(const char *why) { g_last_error = why; return TSX_HIP_EINVAL; }
static int correct_check(const tsx_hip_map *m, const tsx_hip_correct_rule *r) {
    if (!m) return correct_fail("correct: no map");
    if (!r) return correct_fail("correct: no rule");
    if (m->p.lg != m->p.l) return correct_fail("correct: a map created with shard_bits > 0");
    if (m->minq) return correct_fail("correct: a table with min_qual_char set (every low-quality base would be a site for ever)");
    if (r->lower > r->upper) return correct_fail("correct: lower > upper");
    if (r->min_windows < 1 || r->min_windows > (uint32_t)m->p.k) return correct_fail("correct: min_windows outside 1..k");
    if (r->reserved != 0) return correct_fail("correct: reserved must be 0");
    return TSX_HIP_OK;
}

// Sites of a text of `len` bytes: a bound that cannot be exceeded.  A record of n >= 2 windows holds at most
// (n - 3) / (k + 1) + 2 sites (interior runs are k windows long, a solid window between any two runs) and takes at least
// n + k + 2 bytes (a header byte, two line ends, the last of which the text's end may stand for); the ratio is largest
// for n = 2.
static uint64_t correct_site_cap(uint64_t len, int k) { return 2 * len / ((uint64_t)k + 4) + 4; }

// Scratch of one correction call: the map's (bitmap, line offsets, site list, corrections: kept between calls, so that a
// call on a text no larger than an earlier one allocates nothing), the output copy and the piece scratch.
struct CorrectBufs {
    tsx_hip_map::CorrectScratch &s;
    OutBuf out;
    PieceBufs p;
    CorrectBufs(tsx_hip_map *m, hipStream_t st) : s(m->correct), p(st) {}
};

// Behind the bitmap and the line offsets (positions of d_text; records [0, min(cap, *d_nrec or nrec)), the first of them
// record rec_base of the text): the site pass and the probe pass.  tot: CT_N zeroed device words, tot[CT_CORRECTED] the
// cursor of corr (corr_cap entries).  Queued, not waited for.
static int correct_passes(tsx_hip_map *m, CorrectBufs &b, const uint8_t *d_text, uint64_t len, const unsigned long long *bits,
                          const unsigned long long *lo, const unsigned long long *d_nrec, uint64_t nrec, uint64_t cap,
                          uint64_t rec_base, const tsx_hip_correct_rule &rule, CorrectionRec *corr, uint64_t corr_cap,
                          unsigned long long *tot, hipStream_t st) {
    const uint64_t site_cap = correct_site_cap(len, m->p.k);
    TSX_TRY(grow(st, b.s.sites, site_cap * sizeof(CorrectSite)));
    TSX_TRY(grow(st, b.s.nsites, sizeof(unsigned long long)));
    HIP_TRY(hipMemsetAsync(b.s.nsites.get(), 0, sizeof(unsigned long long), st));
    hipLaunchKernelGGL(correct_sites_kernel, dim3(grid_for(m, cap, 8)), dim3(NT), 0, st, bits, lo, d_nrec, nrec, cap,
                       (uint32_t)m->p.k, rule.min_windows, b.s.sites.get(), site_cap, b.s.nsites.get());
    HIP_TRY(hipGetLastError());
    // the probe kernel reads A * (d << 2j) as a LUT entry: a 2-bit field must not straddle a LUT group
    if (m->p.g != 4 && m->p.g != 8) { g_last_error = "correct: a hash LUT of groups other than 4 or 8 bits"; return TSX_HIP_EINVAL; }
    const CorrectArgs ca = {rule.lower, rule.upper, rec_base, len};
    const size_t lut_bytes = m->lut.size() * 8;
    const int grid = (int)std::max<uint64_t>(1, std::min<uint64_t>((site_cap + NT / 64 - 1) / (NT / 64), (uint64_t)m->cus * 8));
#define CORRECT_PROBE(AOV)                                                                                                      \
    DISPATCH_CANON(m, DISPATCH_WK(m, hipLaunchKernelGGL((correct_probe_kernel<WKV, CANV, AOV>), dim3(grid), dim3(NT), lut_bytes, \
                                                        st, m->p, ca, d_text, lo, (const CorrectSite *)b.s.sites.get(),           \
                                                        (const unsigned long long *)b.s.nsites.get(), site_cap, corr, corr_cap, tot)))
    if (m->p.acgt_only) { CORRECT_PROBE(true); } else { CORRECT_PROBE(false); }
#undef CORRECT_PROBE
    HIP_TRY(hipGetLastError());
    return TSX_HIP_OK;
}

static void correct_apply_launch(tsx_hip_map *m, const CorrectionRec *corr, const unsigned long long *n_corr, uint64_t corr_cap,
                                 const unsigned long long *lo, uint64_t rec_base, uint8_t *out, uint64_t out_n,
                                 unsigned long long *total, hipStream_t st) {
    hipLaunchKernelGGL(correct_apply_kernel, dim3(grid_for(m, corr_cap, 8)), dim3(NT), 0, st, corr, n_corr, corr_cap, lo, rec_base,
                       out, out_n, total, out_n);
}

// One piece: piece_front, then over its whole records [0, cut): bitmap, line offsets, sites, probes (totals in
// info[5..7], the corrections in b.corr) and -- `copy` -- the text with them applied in b.out (its size -> info[3]).
// What follows the wait is queued, not waited for.  Not last and no whole record: nrec = 0 and cut = 0, nothing done; a
// last piece without a record (empty lines): nrec = 0, cut = len, and `copy` stages its bytes as they are.
static int correct_piece(tsx_hip_map *m, CorrectBufs &b, const uint8_t *d_text, uint64_t len, bool last, uint64_t rec_base,
                         const tsx_hip_correct_rule &rule, bool copy, hipStream_t st, uint64_t &cut, uint64_t &nrec) {
    bool open;
    TSX_TRY(piece_front(m, b.p, d_text, len, last, false, cut, nrec, open));
    if (nrec == 0) {
        // a last piece of empty lines only: its bytes are output all the same (the apply launch only reports the size)
        if (copy && cut) {
            TSX_TRY(b.out.room(st, cut));
            HIP_TRY(hipMemcpyAsync(b.out.out, d_text, cut, hipMemcpyDeviceToDevice, st));
            correct_apply_launch(m, nullptr, b.p.info.get() + 5 + CT_CORRECTED, 0, nullptr, rec_base, b.out.out, cut, b.p.info.get() + 3, st);
            HIP_TRY(hipGetLastError());
        }
        return TSX_HIP_OK;
    }
    const uint64_t nwords = (cut + 63) / 64, corr_cap = correct_site_cap(cut, m->p.k);
    TSX_TRY(grow(st, b.s.bits, (nwords + 1) * 8));
    TSX_TRY(grow(st, b.s.lo, nrec * TL_N * 8));
    TSX_TRY(grow(st, b.s.corr, corr_cap * sizeof(CorrectionRec)));
    HIP_TRY(hipMemsetAsync(b.s.lo.get(), 0, nrec * TL_N * 8, st));
    const unsigned long long *zero = b.p.info.get() + 4;
    const tsx_hip_trim_rule solid = {rule.lower, rule.upper, 0, TSX_HIP_TRIM_LONGEST, 0};
    TSX_TRY(solid_launch(m, d_text, cut, cut, 0, zero, solid, b.s.bits.get(), st));
    // (the carry is read for an unterminated last line only: then cut = len and it holds the lines of [0, cut))
    lines_launch(m, d_text, cut, cut, 0, zero, 0, last, b.s.lo.get(), nrec, st);
    unsigned long long *tot = b.p.info.get() + 5;
    TSX_TRY(correct_passes(m, b, d_text, cut, b.s.bits.get(), b.s.lo.get(), nullptr, nrec, nrec, rec_base, rule, b.s.corr.get(), corr_cap,
                           tot, st));
    if (copy) {
        TSX_TRY(b.out.room(st, cut));
        HIP_TRY(hipMemcpyAsync(b.out.out, d_text, cut, hipMemcpyDeviceToDevice, st));
        correct_apply_launch(m, b.s.corr.get(), tot + CT_CORRECTED, corr_cap, b.s.lo.get(), rec_base, b.out.out, cut, b.p.info.get() + 3, st);
        HIP_TRY(hipGetLastError());
    }
    return TSX_HIP_OK;
}

static void correct_totals(tsx_hip_correct_totals *t, uint64_t records, const uint64_t *tot, uint64_t bytes) {
    if (t) *t = tsx_hip_correct_totals{records, tot[0] + tot[1] + tot[2], tot[CT_CORRECTED], tot[CT_AMBIGUOUS], tot[CT_UNFIXABLE], bytes};
}

// Sites and corrected reads of a host text: the pieces of host_pieces (at most TSX_HIP_PIECE_BYTES each).  fd < 0: the
// corrections of every piece are gathered and sorted by (record, pos), the first `cap` go to corr_out.  Else the pieces,
// corrected, go to fd through the write-behind.
static int correct_host(tsx_hip_map *m, const char *text, size_t n, const tsx_hip_correct_rule &rule, size_t chunk_bytes,
                        tsx_hip_correction *corr_out, size_t cap, size_t *n_corr, int fd, tsx_hip_correct_totals *totals) {
    hipStream_t st = m->stream.get();
    WriteBehind wb;
    wb.fd = fd;
    std::vector<tsx_hip_correction> all;
    CorrectBufs b(m, st);
    uint64_t records = 0, tot[CT_N] = {0, 0, 0};
    int rc = host_pieces(m, b.p, text, n, chunk_bytes, true, records,
        [&](const uint8_t *d_text, uint64_t len, bool last, uint64_t &cut, uint64_t &nrec, bool &) {
            return correct_piece(m, b, d_text, len, last, records, rule, fd >= 0, st, cut, nrec);
        },
        [&](size_t, uint64_t, uint64_t cut, uint64_t nrec, bool) -> int {
            if (fd >= 0) return cut ? wb.piece(b.p, b.out.out, cut, CT_N, tot, "correct") : TSX_HIP_OK;
            if (!nrec) return TSX_HIP_OK;
            unsigned long long *h = b.p.h_info.get();
            HIP_TRY(hipMemcpyAsync(h + 5, b.p.info.get() + 5, CT_N * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            const uint64_t nc = h[5 + CT_CORRECTED];
            for (int i = 0; i < CT_N; ++i) tot[i] += h[5 + i];
            if (nc) {
                const size_t at = all.size();
                all.resize(at + nc);
                HIP_TRY(hipMemcpyAsync(all.data() + at, b.s.corr.get(), nc * sizeof(tsx_hip_correction), hipMemcpyDeviceToHost, st));
                HIP_TRY(hipStreamSynchronize(st));
            }
            HIP_TRY(hipMemsetAsync(b.p.info.get() + 5, 0, CT_N * sizeof(unsigned long long), st));
            return TSX_HIP_OK;
        });
    if (rc == TSX_HIP_OK) rc = wb.flush();
    correct_totals(totals, records, tot, wb.bytes);
    if (fd < 0) {
        std::sort(all.begin(), all.end(), [](const tsx_hip_correction &x, const tsx_hip_correction &y) {
            return x.record != y.record ? x.record < y.record : x.pos < y.pos;
        });
        if (n_corr) *n_corr = all.size();
        if (corr_out && cap) memcpy(corr_out, all.data(), std::min(all.size(), cap) * sizeof(tsx_hip_correction));
        if (rc == TSX_HIP_OK && all.size() > cap) rc = TSX_HIP_ERANGE;
    }
    return rc;
}

extern "C" int tsx_hip_correct_sites_host(tsx_hip_map *m, const char *text, size_t n, const tsx_hip_correct_rule *rule,
                                          tsx_hip_correction *corrections_out, size_t cap, size_t *n_corrections,
                                          tsx_hip_correct_totals *totals, size_t chunk_bytes) {
    if (n_corrections) *n_corrections = 0;
    if (totals) *totals = tsx_hip_correct_totals{0, 0, 0, 0, 0, 0};
    TSX_TRY(correct_check(m, rule));
    if ((!text && n) || (!corrections_out && cap)) return correct_fail("correct: the text or the corrections pointer");
    return correct_host(m, text, n, *rule, chunk_bytes, corrections_out, cap, n_corrections, -1, totals);
}

extern "C" int tsx_hip_correct_reads_host(tsx_hip_map *m, const char *text, size_t n, const tsx_hip_correct_rule *rule, int fd,
                                          size_t chunk_bytes, tsx_hip_correct_totals *totals) {
    if (totals) *totals = tsx_hip_correct_totals{0, 0, 0, 0, 0, 0};
    TSX_TRY(correct_check(m, rule));
    if ((!text && n) || fd < 0) return correct_fail("correct: the text or the output descriptor");
    return correct_host(m, text, n, *rule, chunk_bytes, nullptr, 0, nullptr, fd, totals);
}

// A device text in windows (device_windows, whole bitmap words, as tsx_hip_trim_spans_device): one bitmap and one array of
// line offsets of the whole text; the sites and the probes once, after the last window.  dev_corr (cap entries, may be
// null with cap 0): the corrections, in no order.  dev_out: the text with them applied (the corrections are then kept in
// scratch, all of them).  WAITS for the stream.
static int correct_device(tsx_hip_map *m, const void *dev_text, size_t n, const tsx_hip_correct_rule &rule, void *dev_corr,
                          size_t cap, size_t *n_corr, void *dev_out, tsx_hip_correct_totals *totals, void *stream) {
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t st = pick_stream(m, stream);
    TSX_TRY(ensure_zeroed(m, st));
    const uint64_t rcap = max_records(m, n), nwords = ((uint64_t)n + 63) / 64;
    CorrectBufs b(m, st);
    DevBuf<unsigned long long> &tot = b.s.tot;
    SyncAtExit wait(st);
    TSX_TRY(grow(st, b.s.bits, (nwords + 1) * 8));
    TSX_TRY(grow(st, b.s.lo, (rcap + 1) * TL_N * 8));
    TSX_TRY(grow(st, tot, CT_N * 8));
    HIP_TRY(hipMemsetAsync(b.s.lo.get(), 0, (rcap + 1) * TL_N * 8, st));
    HIP_TRY(hipMemsetAsync(tot.get(), 0, CT_N * 8, st));
    const uint8_t *base = (const uint8_t *)dev_text;
    const tsx_hip_trim_rule solid = {rule.lower, rule.upper, 0, TSX_HIP_TRIM_LONGEST, 0};
    TSX_TRY(device_windows(m, base, n, true, st,
                           [&](size_t off, size_t own, size_t len, int head_open, bool last, const unsigned long long *d_base) -> int {
                               TSX_TRY(solid_launch(m, base + off, len, own, head_open, d_base, solid, b.s.bits.get() + off / 64, st));
                               lines_launch(m, base + off, len, own, head_open, d_base, off, last, b.s.lo.get(), rcap, st);
                               return TSX_HIP_OK;
                           }));
    CorrectionRec *corr = (CorrectionRec *)dev_corr;
    uint64_t corr_cap = cap;
    if (dev_out) {
        corr_cap = correct_site_cap(n, m->p.k);
        TSX_TRY(grow(st, b.s.corr, corr_cap * sizeof(CorrectionRec)));
        corr = b.s.corr.get();
    }
    unsigned long long h[CT_N + 1] = {0, 0, 0, 0};
    if (n) {
        const unsigned long long *d_nrec = (const unsigned long long *)m->d_carry.get() + 3;
        TSX_TRY(correct_passes(m, b, base, n, b.s.bits.get(), b.s.lo.get(), d_nrec, 0, rcap, 0, rule, corr, corr_cap, tot.get(), st));
        if (dev_out) {
            if (dev_out != dev_text) HIP_TRY(hipMemcpyAsync(dev_out, dev_text, n, hipMemcpyDeviceToDevice, st));
            correct_apply_launch(m, corr, tot.get() + CT_CORRECTED, corr_cap, b.s.lo.get(), 0, (uint8_t *)dev_out, n, nullptr, st);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipMemcpyAsync(h, tot.get(), CT_N * 8, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipMemcpyAsync(h + CT_N, (const unsigned long long *)m->d_carry.get() + 3, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const uint64_t t3[CT_N] = {h[0], h[1], h[2]};
    correct_totals(totals, h[CT_N], t3, dev_out ? n : 0);
    if (n_corr) *n_corr = (size_t)h[CT_CORRECTED];
    return (!dev_out && h[CT_CORRECTED] > cap) ? TSX_HIP_ERANGE : TSX_HIP_OK;
}

extern "C" int tsx_hip_correct_sites_device(tsx_hip_map *m, const void *dev_text, size_t n, const tsx_hip_correct_rule *rule,
                                            void *dev_corrections, size_t cap, size_t *n_corrections,
                                            tsx_hip_correct_totals *totals, void *stream) {
    if (n_corrections) *n_corrections = 0;
    if (totals) *totals = tsx_hip_correct_totals{0, 0, 0, 0, 0, 0};
    TSX_TRY(correct_check(m, rule));
    if ((!dev_text && n) || ((uintptr_t)dev_text & 15) || (!dev_corrections && cap) || ((uintptr_t)dev_corrections & 7))
        return correct_fail("correct: the text (16-byte aligned) or the corrections pointer");
    return correct_device(m, dev_text, n, *rule, dev_corrections, cap, n_corrections, nullptr, totals, stream);
}

extern "C" int tsx_hip_correct_reads_device(tsx_hip_map *m, const void *dev_text, size_t n, const tsx_hip_correct_rule *rule,
                                            void *dev_out, size_t out_cap, tsx_hip_correct_totals *totals, void *stream) {
    if (totals) *totals = tsx_hip_correct_totals{0, 0, 0, 0, 0, 0};
    TSX_TRY(correct_check(m, rule));
    if ((!dev_text && n) || ((uintptr_t)dev_text & 15) || !dev_out)
        return correct_fail("correct: the text (16-byte aligned) or the output pointer");
    if (out_cap < n) return TSX_HIP_ERANGE;
    return correct_device(m, dev_text, n, *rule, nullptr, 0, nullptr, dev_out, totals, stream);
}

// ---- read medians: the count of every window, the median of every record, the filter on it (tsx_median.h) ---------
static const uint64_t MEDIAN_LONG_DEFAULT = 16384;   // bases of a sequence line above which a workgroup selects

// TSX_HIP_MEDIAN_LONG, read per call (tests send reads through the workgroup form): at least 64.
static uint64_t median_long_bases() {
    uint64_t v = MEDIAN_LONG_DEFAULT;
    if (const char *e = getenv("TSX_HIP_MEDIAN_LONG")) {
        const long long x = atoll(e);
        if (x >= 64) v = (uint64_t)x;
    }
    return v;
}

static bool median_rule_ok(const tsx_hip_median_rule *r) { return r && r->lower <= r->upper && r->reserved == 0; }

// A range of the tiles of a text that has had its line pass: the tiles [first, first + count) of tile_line (NULL: the
// map's d_tile).  ALL_TILES: every tile of the launch, what the calls on whole pieces and windows pass.
struct TileSpan { uint64_t first, count; const uint32_t *tile_line; };
static const TileSpan ALL_TILES = {0, ~0ULL, nullptr};

// window_counts_kernel over the start positions [0, own_end) of d_text (n readable bytes), after line_pass: those of the
// tiles `ts`.
static int counts_launch(tsx_hip_map *m, const uint8_t *d_text, uint64_t n, uint64_t own_end, int head_open,
                         const unsigned long long *d_line_base, uint32_t *d_profile, const TileSpan &ts, hipStream_t st) {
    if (own_end == 0 || ts.count == 0) return TSX_HIP_OK;
    const uint64_t ntiles = (own_end + TILE - 1) / TILE;
    const uint64_t t0 = std::min(ts.first, ntiles), t1 = t0 + std::min(ts.count, ntiles - t0);
    if (t0 == t1) return TSX_HIP_OK;
    const uint32_t *tile_line = ts.tile_line ? ts.tile_line : (const uint32_t *)m->d_tile.get();
    const size_t lut_bytes = m->lut.size() * 8;
    const int grid = (int)std::min<uint64_t>(t1 - t0, (uint64_t)m->cus * 4);
    DISPATCH_BR(m, DISPATCH_CANON(m, DISPATCH_WK(m, hipLaunchKernelGGL((window_counts_kernel<WKV, CANV, BRV>), dim3(grid), dim3(NT),
                                                        lut_bytes, st, m->p, d_text, n, own_end, head_open, tile_line, t0, t1,
                                                        d_line_base, d_profile, m->qmap_cur))));
    HIP_TRY(hipGetLastError());
    return TSX_HIP_OK;
}

// Entries of the list of long records for a text of n bytes (the counter in front of them not counted).
static uint64_t median_list_cap(uint64_t n, uint64_t long_len) { return n / (long_len + 1) + 2; }

// Both selection kernels over the records [rec0, min(cap, *d_nrec or nrec)) with line offsets in lo: the wave form lists
// the long records (list: the counter, then list_cap entries), the workgroup form takes them.  Queued, not waited for.
static int median_select(tsx_hip_map *m, const uint32_t *d_profile, const unsigned long long *lo, const unsigned long long *d_nrec,
                         uint64_t rec0, uint64_t nrec, uint64_t cap, uint64_t long_len, unsigned long long *list, uint64_t list_cap,
                         unsigned long long *med, hipStream_t st) {
    if (cap <= rec0) return TSX_HIP_OK;
    HIP_TRY(hipMemsetAsync(list, 0, sizeof(unsigned long long), st));
    hipLaunchKernelGGL(median_select_kernel, dim3((uint32_t)std::min<uint64_t>(cap - rec0, (uint64_t)m->cus * 32)), dim3(64), 0, st,
                       d_profile, lo, d_nrec, rec0, nrec, cap, (uint32_t)m->p.k, long_len, list, list_cap, med);
    hipLaunchKernelGGL(median_select_long_kernel, dim3((uint32_t)std::min<uint64_t>(list_cap, (uint64_t)m->cus * 4)), dim3(NT), 0, st,
                       d_profile, lo, (const unsigned long long *)list, list_cap, (uint32_t)m->p.k, med);
    HIP_TRY(hipGetLastError());
    return TSX_HIP_OK;
}

// The windows of a device text (device_windows, whole 64-byte words as tsx_hip_trim_spans_device walks them): every window
// writes its part of the profile and, when `lo` is given, its line offsets (records < cap).
static int median_windows(tsx_hip_map *m, const uint8_t *base, size_t n, uint32_t *d_profile, unsigned long long *lo, uint64_t cap,
                          hipStream_t st) {
    return device_windows(m, base, n, true, st,
                          [&](size_t off, size_t own, size_t len, int head_open, bool last, const unsigned long long *d_base) -> int {
                              TSX_TRY(counts_launch(m, base + off, len, own, head_open, d_base, d_profile + off, ALL_TILES, st));
                              if (lo) lines_launch(m, base + off, len, own, head_open, d_base, off, last, lo, cap, st);
                              return TSX_HIP_OK;
                          });
}

extern "C" int tsx_hip_count_profile_device(tsx_hip_map *m, const void *dev_text, size_t n, void *dev_profile, void *stream) {
    if (!query_args_ok(m, 0, 0) || (!dev_text && n) || ((uintptr_t)dev_text & 15) || (!dev_profile && n) || ((uintptr_t)dev_profile & 3))
        return TSX_HIP_EINVAL;
    hipStream_t st;
    TSX_TRY(device_begin(m, stream, st));
    SyncAtExit wait(st);
    TSX_TRY(median_windows(m, (const uint8_t *)dev_text, n, (uint32_t *)dev_profile, nullptr, 0, st));
    HIP_TRY(hipStreamSynchronize(st));
    return TSX_HIP_OK;
}

// The profile of the whole text and the line offsets stay on the device until the last window; then one selection.
extern "C" int tsx_hip_median_reads_device(tsx_hip_map *m, const void *dev_text, size_t n, void *dev_medians, size_t med_cap,
                                           size_t *n_records, void *stream) {
    if (n_records) *n_records = 0;
    if (!query_args_ok(m, 0, 0) || (!dev_text && n) || ((uintptr_t)dev_text & 15) || (!dev_medians && med_cap) ||
        ((uintptr_t)dev_medians & 7))
        return TSX_HIP_EINVAL;
    hipStream_t st;
    TSX_TRY(device_begin(m, stream, st));
    const uint64_t cap = std::min<uint64_t>(med_cap, max_records(m, n));
    const uint64_t long_len = median_long_bases(), list_cap = median_list_cap(n, long_len);
    DevBuf<uint32_t> profile;
    DevBuf<unsigned long long> lo, list;
    SyncAtExit wait(st);
    TSX_TRY(profile.alloc(((size_t)n + 16) * sizeof(uint32_t)));
    TSX_TRY(lo.alloc((cap + 1) * TL_N * 8));
    TSX_TRY(list.alloc((list_cap + 1) * 8));
    HIP_TRY(hipMemsetAsync(lo.get(), 0, (cap + 1) * TL_N * 8, st));
    TSX_TRY(median_windows(m, (const uint8_t *)dev_text, n, profile.get(), lo.get(), cap, st));
    const unsigned long long *d_nrec = (const unsigned long long *)m->d_carry.get() + 3;
    TSX_TRY(median_select(m, profile.get(), lo.get(), d_nrec, 0, 0, cap, long_len, list.get(), list_cap, (unsigned long long *)dev_medians, st));
    unsigned long long nrec = 0;
    HIP_TRY(hipMemcpyAsync(&nrec, d_nrec, sizeof nrec, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (n_records) *n_records = (size_t)nrec;
    return nrec > med_cap ? TSX_HIP_ERANGE : TSX_HIP_OK;
}

// Scratch of one median call that works on pieces.
struct MedianBufs {
    DevBuf<uint32_t> profile;
    DevBuf<unsigned long long> lo, list, med;
    Compaction c;      // the filter's kept lengths and its output
    PieceBufs p;
    explicit MedianBufs(hipStream_t s) : p(s) {}
};

enum { MED_PROFILE = 0, MED_MEDIANS = 1, MED_FILTER = 2 };

// One piece: piece_front, then over its whole records [0, cut) the profile in b.profile and -- unless only the profile
// is asked for -- the line offsets and the medians in b.med.  What follows the wait is queued, not waited for.  Not last
// and no whole record: nrec = 0, nothing done.
static int median_piece(tsx_hip_map *m, MedianBufs &b, const uint8_t *d_text, uint64_t len, bool last, int what, uint64_t long_len,
                        hipStream_t st, uint64_t &cut, uint64_t &nrec, bool &open) {
    TSX_TRY(piece_front(m, b.p, d_text, len, last, what == MED_FILTER, cut, nrec, open));
    if (nrec == 0) return TSX_HIP_OK;
    TSX_TRY(grow(st, b.profile, (cut + 16) * sizeof(uint32_t)));
    QmapScope qs(m);
    TSX_TRY(piece_qmap(m, d_text, cut, st));
    const unsigned long long *zero = b.p.info.get() + 4;
    TSX_TRY(counts_launch(m, d_text, cut, cut, 0, zero, b.profile.get(), ALL_TILES, st));
    if (what == MED_PROFILE) return TSX_HIP_OK;
    const uint64_t list_cap = median_list_cap(cut, long_len);
    TSX_TRY(grow(st, b.lo, nrec * TL_N * 8));
    TSX_TRY(grow(st, b.med, nrec * sizeof(tsx_hip_read_median)));
    TSX_TRY(grow(st, b.list, (list_cap + 1) * 8));
    HIP_TRY(hipMemsetAsync(b.lo.get(), 0, nrec * TL_N * 8, st));
    // (the carry is read for an unterminated last line only: then cut = len and it holds the lines of [0, cut))
    lines_launch(m, d_text, cut, cut, 0, zero, 0, last, b.lo.get(), nrec, st);
    return median_select(m, b.profile.get(), b.lo.get(), nullptr, 0, nrec, nrec, long_len, b.list.get(), list_cap, b.med.get(), st);
}

// The median filter behind median_piece, as filter_piece: kept lengths by the medians, their scan (total -> info[3], kept
// records -> info[5]), the compaction into b.c.out.  Queued, not waited for.
static int median_filter_piece(tsx_hip_map *m, MedianBufs &b, const uint8_t *d_text, uint64_t cut, uint64_t nrec, bool open,
                               const tsx_hip_median_rule &rule, hipStream_t st) {
    unsigned long long *koff, *const info = b.p.info.get();
    const unsigned long long *span = b.p.rspan.get();
    TSX_TRY(b.c.lengths(st, nrec, koff));
    hipLaunchKernelGGL(median_len_kernel, dim3(grid_for(m, nrec, 8)), dim3(NT), 0, st, (const unsigned long long *)b.med.get(),
                       span, nrec, rule.lower, rule.upper, rule.invert, open ? 1 : 0, koff, info + 5);
    return b.c.copy_spans(m, d_text, cut, span, nrec, info + 3, st);
}

// Profile, medians and the median filter: the pieces of host_pieces, at most TSX_HIP_PIECE_BYTES each when that is set.
// MED_PROFILE: each piece's profile goes to profile_out + its offset.  MED_MEDIANS: each piece's medians go to
// med_out[rec_base ..] while they fit.  MED_FILTER: write-behind to fd.
static int median_host(tsx_hip_map *m, const char *text, size_t n, int what, size_t chunk_bytes, uint32_t *profile_out,
                       tsx_hip_read_median *med_out, size_t med_cap, size_t *n_records, const tsx_hip_median_rule *rule, int fd,
                       uint64_t *kept_out, uint64_t *bytes_out) {
    hipStream_t st = m->stream.get();
    WriteBehind wb;
    wb.fd = fd;
    MedianBufs b(st);
    const uint64_t long_len = median_long_bases();
    uint64_t rec_base = 0, kept = 0;
    int rc = host_pieces(m, b.p, text, n, chunk_bytes, true, rec_base,
        [&](const uint8_t *d_text, uint64_t len, bool last, uint64_t &cut, uint64_t &nrec, bool &open) {
            return median_piece(m, b, d_text, len, last, what, long_len, st, cut, nrec, open);
        },
        [&](size_t off, uint64_t base, uint64_t cut, uint64_t nrec, bool open) -> int {
            if (what == MED_MEDIANS) return deliver_records(med_out, med_cap, base, b.med.get(), nrec, st);
            if (what == MED_PROFILE) {
                if (nrec) {
                    HIP_TRY(hipMemcpyAsync(profile_out + off, b.profile.get(), cut * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
                    HIP_TRY(hipStreamSynchronize(st));
                } else {   // (a last piece without a record holds empty lines only)
                    std::fill(profile_out + off, profile_out + off + cut, (uint32_t)TSX_HIP_NO_KMER);
                }
                return TSX_HIP_OK;
            }
            if (!nrec) return TSX_HIP_OK;
            TSX_TRY(median_filter_piece(m, b, b.p.text.get(), cut, nrec, open, *rule, st));
            return wb.piece(b.p, b.c.out.out, cut, 1, &kept, "filter");
        });
    if (rc == TSX_HIP_OK) rc = wb.flush();
    if (n_records) *n_records = (size_t)rec_base;
    if (kept_out) *kept_out = kept;
    if (bytes_out) *bytes_out = wb.bytes;
    if (rc == TSX_HIP_OK && what == MED_MEDIANS && rec_base > med_cap) rc = TSX_HIP_ERANGE;
    return rc;
}

extern "C" int tsx_hip_count_profile_host(tsx_hip_map *m, const char *text, size_t n, uint32_t *profile_out, size_t chunk_bytes) {
    if (!query_args_ok(m, 0, 0) || (!text && n) || (!profile_out && n)) return TSX_HIP_EINVAL;
    return median_host(m, text, n, MED_PROFILE, chunk_bytes, profile_out, nullptr, 0, nullptr, nullptr, -1, nullptr, nullptr);
}

extern "C" int tsx_hip_median_reads_host(tsx_hip_map *m, const char *text, size_t n, tsx_hip_read_median *out, size_t cap,
                                         size_t *n_records, size_t chunk_bytes) {
    if (n_records) *n_records = 0;
    if (!query_args_ok(m, 0, 0) || (!text && n) || (!out && cap)) return TSX_HIP_EINVAL;
    return median_host(m, text, n, MED_MEDIANS, chunk_bytes, nullptr, out, cap, n_records, nullptr, -1, nullptr, nullptr);
}

extern "C" int tsx_hip_filter_median_host(tsx_hip_map *m, const char *text, size_t n, const tsx_hip_median_rule *rule, int fd,
                                          size_t chunk_bytes, uint64_t *kept_out, uint64_t *bytes_out) {
    if (kept_out) *kept_out = 0;
    if (bytes_out) *bytes_out = 0;
    if (!median_rule_ok(rule) || !query_args_ok(m, 0, 0) || (!text && n) || fd < 0) return TSX_HIP_EINVAL;
    return median_host(m, text, n, MED_FILTER, chunk_bytes, nullptr, nullptr, 0, nullptr, rule, fd, kept_out, bytes_out);
}

// ---- digital normalization: rounds of records judged by their medians, the kept ones counted (tsx_normalize.h) ----
// What the atomic insert path into a whole table asks of the map and the rule.  No GPU call.
static int normalize_args_ok(const tsx_hip_map *m, const tsx_hip_normalize_rule *r) {
    if (!m) return TSX_HIP_EINVAL;
    if (m->p.lg != m->p.l) { g_last_error = "normalize: a map created with shard_bits > 0"; return TSX_HIP_EINVAL; }
    if (slab_bits(m)) { g_last_error = "normalize: a table above 2^32 slots is built slab by slab, not by the atomic path"; return TSX_HIP_EINVAL; }
    if (m->pf_armed) { g_last_error = "normalize: a prefilter is armed"; return TSX_HIP_EINVAL; }
    if (!r) { g_last_error = "normalize: no rule"; return TSX_HIP_EINVAL; }
    if (r->round_records == 0) { g_last_error = "normalize: round_records = 0"; return TSX_HIP_EINVAL; }
    if (r->reserved[0] || r->reserved[1]) { g_last_error = "normalize: reserved != 0"; return TSX_HIP_EINVAL; }
    return TSX_HIP_OK;
}

// A window of a text whose line pass is kept: `own` start positions from byte `off` of the whole text (len readable
// bytes), the tile line counts and the line base the pass left, the window's part of a quality bitmap.  A host piece is
// one such window at off 0.
struct NormWindow {
    const uint8_t *text;
    uint64_t off, own, len;
    int head_open;
    const uint32_t *tile_line;
    const unsigned long long *line_base;
    const uint16_t *qmap;
};

// Scratch of a normalization that both forms use.
struct NormBufs {
    DevBuf<uint32_t> keep;                         // one bit per record
    DevBuf<unsigned long long> bounds, tiles;      // where the rounds start; tiles the gate skipped
    PinBuf<unsigned long long> h_bounds;
    uint64_t covered = 0;                          // tiles the count launches covered
};

// count_kept_kernel over the tiles [t0, t1) of a window, for the records [r0, r1).
static int kept_launch(tsx_hip_map *m, const NormWindow &w, uint64_t t0, uint64_t t1, const uint32_t *keep, uint64_t r0,
                       uint64_t r1, unsigned long long *skipped, hipStream_t st) {
    const size_t lut_bytes = m->lut.size() * 8;
    const int grid = (int)std::min<uint64_t>(t1 - t0, (uint64_t)m->cus * 3);
    const uint64_t tiles_all = (w.own + TILE - 1) / TILE;
    const uint32_t lshift = line_shift(m);
    DISPATCH_BR(m, DISPATCH_CANON(m, DISPATCH_WK(m, hipLaunchKernelGGL((count_kept_kernel<WKV, CANV, BRV>), dim3(grid), dim3(NT),
                                                        lut_bytes, st, m->p, w.text, w.len, w.own, w.head_open, w.tile_line, t0, t1,
                                                        tiles_all, w.line_base, lshift, keep, r0, r1, skipped, m->qmap_cur))));
    HIP_TRY(hipGetLastError());
    return TSX_HIP_OK;
}

// The rounds of the records [0, nrec) of a text that lies in the windows win[0, nwin) (in text order; its records end
// at byte `end`), R records each: per round the profile of its tiles, the medians of its records, the keep rule, the
// count of the kept.  profile: the entry of byte 0 of the text; lo: the line offsets of the records (text positions).
// span / len: the record spans and the kept lengths for Compaction::copy_spans (both NULL: no output); keep_bytes: one
// byte per record < bytes_cap, or NULL.  totals: NT_N device words that grow.  Waits once, for the round bounds; the rounds are
// queued.  The caller holds a QmapScope.
static int normalize_rounds(tsx_hip_map *m, NormBufs &nb, const NormWindow *win, size_t nwin, uint64_t end, uint64_t nrec, uint64_t R,
                            uint64_t cutoff, uint32_t *profile, const unsigned long long *lo, const unsigned long long *span,
                            unsigned long long *len, bool nl_last, uint8_t *keep_bytes, uint64_t bytes_cap,
                            unsigned long long *list, uint64_t list_cap, unsigned long long *med, unsigned long long *totals,
                            uint64_t long_len, hipStream_t st, uint64_t &rounds) {
    if (nrec == 0) return TSX_HIP_OK;
    const uint64_t nrounds = (nrec - 1) / R + 1;
    TSX_TRY(grow(st, nb.keep, ((nrec + 31) / 32 + 1) * sizeof(uint32_t)));
    TSX_TRY(grow(st, nb.bounds, (nrounds + 1) * 8));
    TSX_TRY(nb.h_bounds.reserve(&st, (nrounds + 1) * 8, (nrounds + 1) * 8 + 4096));
    HIP_TRY(hipMemsetAsync(nb.keep.get(), 0, ((nrec + 31) / 32 + 1) * sizeof(uint32_t), st));
    hipLaunchKernelGGL(round_bounds_kernel, dim3(grid_for(m, nrounds + 1, 8)), dim3(NT), 0, st, lo, (uint64_t)0, R, nrounds, end,
                       nb.bounds.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(nb.h_bounds.get(), nb.bounds.get(), (nrounds + 1) * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const unsigned long long *hb = nb.h_bounds.get();
    size_t w0 = 0;   // the first window that reaches into the round
    for (uint64_t j = 0; j < nrounds; ++j) {
        const uint64_t r0 = j * R, r1 = nrec - r0 > R ? r0 + R : nrec, b0 = hb[j], b1 = hb[j + 1];
        while (w0 + 1 < nwin && win[w0].off + win[w0].own <= b0) ++w0;
        // the window's tiles that hold start positions of [b0, b1)
        auto tiles_of = [&](const NormWindow &w, uint64_t &t0, uint64_t &t1) {
            const uint64_t a = std::max(b0, w.off) - w.off, b = std::min(b1, w.off + w.own) - w.off;
            t0 = a / TILE; t1 = (b + TILE - 1) / TILE;
        };
        for (size_t wi = w0; wi < nwin && win[wi].off < b1; ++wi) {
            const NormWindow &w = win[wi];
            uint64_t t0, t1;
            tiles_of(w, t0, t1);
            m->qmap_cur = w.qmap;
            TSX_TRY(counts_launch(m, w.text, w.len, w.own, w.head_open, w.line_base, profile + w.off, TileSpan{t0, t1 - t0, w.tile_line}, st));
        }
        TSX_TRY(median_select(m, profile, lo, nullptr, r0, r1, r1, long_len, list, list_cap, med, st));
        hipLaunchKernelGGL(normalize_keep_kernel, dim3(grid_for(m, r1 - r0, 8)), dim3(NT), 0, st, (const unsigned long long *)med, span,
                           r0, r1, nrec, cutoff, nl_last ? 1 : 0, nb.keep.get(), len, keep_bytes, bytes_cap, totals);
        HIP_TRY(hipGetLastError());
        if (cutoff == 0) continue;   // (nothing is kept: nothing to count)
        for (size_t wi = w0; wi < nwin && win[wi].off < b1; ++wi) {
            const NormWindow &w = win[wi];
            uint64_t t0, t1;
            tiles_of(w, t0, t1);
            if (t0 == t1) continue;
            m->qmap_cur = w.qmap;
            TSX_TRY(kept_launch(m, w, t0, t1, nb.keep.get(), r0, r1, nb.tiles.get(), st));
            nb.covered += t1 - t0;
        }
    }
    rounds += nrounds;
    return TSX_HIP_OK;
}

// What both forms do first and last with the gate's tile counters (tsx_hip_debug_counters).
static int normalize_tiles_begin(NormBufs &nb, hipStream_t st) {
    TSX_TRY(nb.tiles.alloc(sizeof(unsigned long long)));
    HIP_TRY(hipMemsetAsync(nb.tiles.get(), 0, sizeof(unsigned long long), st));
    return TSX_HIP_OK;
}
static int normalize_tiles_end(tsx_hip_map *m, NormBufs &nb, hipStream_t st) {
    unsigned long long sk = 0;
    HIP_TRY(hipMemcpyAsync(&sk, nb.tiles.get(), sizeof sk, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    m->norm_tiles = nb.covered; m->norm_skipped = sk;
    return TSX_HIP_OK;
}

// The host form: the pieces of host_pieces, each cut back to its last whole round -- rounds are numbered from the
// record index over the whole text, every piece starts at a multiple of R, and what lies behind the cut is the head of
// the next piece.  A piece that holds no whole round grows, as one that holds no whole record does (host_pieces:
// nrec = 0), so a round longer than a piece is taken whole; the last piece takes what is left, a short round included.
// Compaction and write-behind once per piece.
static int normalize_host(tsx_hip_map *m, const char *text, size_t n, const tsx_hip_normalize_rule &rule, int fd, uint8_t *keep_out,
                          size_t keep_cap, size_t chunk_bytes, tsx_hip_normalize_totals &tot) {
    hipStream_t st = m->stream.get();
    WriteBehind wb;
    wb.fd = fd;
    NormBufs nb;
    DevBuf<uint8_t> keepb;
    MedianBufs b(st);
    const uint64_t long_len = median_long_bases(), R = rule.round_records;
    uint64_t rec_base = 0, count[NT_N] = {0, 0, 0}, rounds = 0;
    bool began = false;
    int rc = host_pieces(m, b.p, text, n, chunk_bytes, true, rec_base,
        [&](const uint8_t *d_text, uint64_t len, bool last, uint64_t &cut, uint64_t &nrec, bool &open) -> int {
            TSX_TRY(piece_front(m, b.p, d_text, len, last, true, cut, nrec, open));
            const uint64_t whole = nrec / R * R;
            if (last || whole == nrec) return TSX_HIP_OK;
            if (whole == 0) { cut = 0; nrec = 0; return TSX_HIP_OK; }   // no whole round: the piece grows
            unsigned long long c = 0;   // record `whole` starts the next piece
            HIP_TRY(hipMemcpyAsync(&c, b.p.rspan.get() + 2 * whole, sizeof c, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            cut = c; nrec = whole; open = false;
            return TSX_HIP_OK;
        },
        [&](size_t, uint64_t base, uint64_t cut, uint64_t nrec, bool open) -> int {
            if (!nrec) return TSX_HIP_OK;
            if (!began) { TSX_TRY(normalize_tiles_begin(nb, st)); began = true; }
            const uint8_t *d_text = b.p.text.get();
            const uint64_t list_cap = median_list_cap(cut, long_len);
            unsigned long long *koff = nullptr;   // the kept lengths, when there is an output
            TSX_TRY(grow(st, b.profile, (cut + 16) * sizeof(uint32_t)));
            TSX_TRY(grow(st, b.lo, nrec * TL_N * 8));
            TSX_TRY(grow(st, b.med, nrec * sizeof(tsx_hip_read_median)));
            TSX_TRY(grow(st, b.list, (list_cap + 1) * 8));
            if (fd >= 0) TSX_TRY(b.c.lengths(st, nrec, koff));
            if (keep_out) TSX_TRY(grow(st, keepb, nrec));
            QmapScope qs(m);
            TSX_TRY(piece_qmap(m, d_text, cut, st));
            unsigned long long *const info = b.p.info.get();
            HIP_TRY(hipMemsetAsync(b.lo.get(), 0, nrec * TL_N * 8, st));
            // (the carry is read for an unterminated last line only: then the piece is the last one, whole)
            lines_launch(m, d_text, cut, cut, 0, info + 4, 0, open, b.lo.get(), nrec, st);
            const NormWindow w = {d_text, 0, cut, cut, 0, (const uint32_t *)m->d_tile.get(), info + 4, m->qmap_cur};
            TSX_TRY(normalize_rounds(m, nb, &w, 1, cut, nrec, R, rule.cutoff, b.profile.get(), b.lo.get(),
                                     fd >= 0 ? b.p.rspan.get() : nullptr, koff, open,
                                     keep_out ? keepb.get() : nullptr, nrec, b.list.get(), list_cap, b.med.get(), info + 5, long_len, st,
                                     rounds));
            if (fd >= 0) {
                TSX_TRY(b.c.copy_spans(m, d_text, cut, b.p.rspan.get(), nrec, info + 3, st));
                TSX_TRY(wb.piece(b.p, b.c.out.out, cut, NT_N, count, "normalize"));
            } else {
                unsigned long long *h = b.p.h_info.get();
                HIP_TRY(hipMemcpyAsync(h + 5, info + 5, NT_N * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
                HIP_TRY(hipStreamSynchronize(st));
                for (int i = 0; i < NT_N; ++i) count[i] += h[5 + i];
                HIP_TRY(hipMemsetAsync(info + 5, 0, NT_N * sizeof(unsigned long long), st));
            }
            return deliver_records(keep_out, keep_out ? keep_cap : 0, base, keepb.get(), nrec, st);
        });
    if (rc == TSX_HIP_OK) rc = wb.flush();
    if (began) { const int rc2 = normalize_tiles_end(m, nb, st); if (rc == TSX_HIP_OK) rc = rc2; }
    tot.records = rec_base; tot.kept = count[NT_KEPT]; tot.kmers_seen = count[NT_SEEN]; tot.kmers_added = count[NT_ADDED];
    tot.rounds = rounds;
    if (rc == TSX_HIP_OK && keep_out && rec_base > keep_cap) rc = TSX_HIP_ERANGE;
    return rc;
}

extern "C" int tsx_hip_normalize_host(tsx_hip_map *m, const char *text, size_t n, const tsx_hip_normalize_rule *rule, int fd,
                                      uint8_t *keep_out, size_t keep_cap, size_t chunk_bytes, tsx_hip_normalize_totals *totals) {
    tsx_hip_normalize_totals tot = {0, 0, 0, 0, 0};
    if (totals) *totals = tot;
    TSX_TRY(normalize_args_ok(m, rule));
    if ((!text && n) || (!keep_out && keep_cap)) return TSX_HIP_EINVAL;
    m->norm_tiles = m->norm_skipped = 0;
    if (n && rule->cutoff) m->used = true;
    const int rc = normalize_host(m, text, n, *rule, fd, keep_out, keep_cap, chunk_bytes, tot);
    if (totals) *totals = tot;
    return rc;
}

// The device form.  device_windows makes the line pass of every window; its tile line counts, its line base and the
// line offsets of its records are kept for the whole text, so that a round -- records by their index over the whole
// text, wherever the window seams fall -- finds the tiles of each window it reaches into.  Then the rounds, as for a
// host piece.
extern "C" int tsx_hip_normalize_device(tsx_hip_map *m, const void *dev_text, size_t n, const tsx_hip_normalize_rule *rule,
                                        void *dev_keep, size_t keep_cap, tsx_hip_normalize_totals *totals, void *stream) {
    tsx_hip_normalize_totals tot = {0, 0, 0, 0, 0};
    if (totals) *totals = tot;
    TSX_TRY(normalize_args_ok(m, rule));
    if ((!dev_text && n) || ((uintptr_t)dev_text & 15) || (!dev_keep && keep_cap)) return TSX_HIP_EINVAL;
    m->norm_tiles = m->norm_skipped = 0;
    if (n && rule->cutoff) m->used = true;
    hipStream_t st;
    TSX_TRY(device_begin(m, stream, st));
    const uint8_t *base = (const uint8_t *)dev_text;
    const uint64_t cap = max_records(m, n);
    const uint64_t long_len = median_long_bases(), list_cap = median_list_cap(n, long_len);
    const size_t WIN = (dev_window_bytes() + 63) & ~(size_t)63, nwin = n ? (n - 1) / WIN + 1 : 0;
    const uint64_t tiles_win = (WIN + TILE - 1) / TILE;   // room per window
    NormBufs nb;
    DevBuf<uint32_t> profile, tile_all;
    DevBuf<unsigned long long> lo, list, med, bases, totals_d;
    SyncAtExit wait(st);
    TSX_TRY(normalize_tiles_begin(nb, st));
    TSX_TRY(profile.alloc(((size_t)n + 16) * sizeof(uint32_t)));
    TSX_TRY(lo.alloc((cap + 1) * TL_N * 8));
    TSX_TRY(list.alloc((list_cap + 1) * 8));
    TSX_TRY(med.alloc((cap + 1) * sizeof(tsx_hip_read_median)));
    TSX_TRY(tile_all.alloc((nwin * tiles_win + 1) * sizeof(uint32_t)));
    TSX_TRY(bases.alloc((nwin + 1) * 8));
    TSX_TRY(totals_d.alloc(NT_N * 8));
    HIP_TRY(hipMemsetAsync(lo.get(), 0, (cap + 1) * TL_N * 8, st));
    HIP_TRY(hipMemsetAsync(totals_d.get(), 0, NT_N * 8, st));
    std::vector<NormWindow> win;
    int rc = device_windows(m, base, n, true, st,
                            [&](size_t off, size_t own, size_t len, int head_open, bool last, const unsigned long long *d_base) -> int {
                                const size_t wi = win.size();
                                uint32_t *tl = tile_all.get() + wi * tiles_win;
                                lines_launch(m, base + off, len, own, head_open, d_base, off, last, lo.get(), cap, st);
                                HIP_TRY(hipMemcpyAsync(tl, m->d_tile.get(), ((own + TILE - 1) / TILE) * sizeof(uint32_t),
                                                       hipMemcpyDeviceToDevice, st));
                                HIP_TRY(hipMemcpyAsync(bases.get() + wi, d_base, 8, hipMemcpyDeviceToDevice, st));
                                win.push_back(NormWindow{base + off, off, own, len, head_open, tl, bases.get() + wi, m->qmap_cur});
                                return TSX_HIP_OK;
                            });
    if (rc != TSX_HIP_OK) return rc;
    unsigned long long nrec = 0;
    HIP_TRY(hipMemcpyAsync(&nrec, (const unsigned long long *)m->d_carry.get() + 3, sizeof nrec, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    uint64_t rounds = 0;
    {
        QmapScope qs(m);
        rc = normalize_rounds(m, nb, win.data(), win.size(), n, nrec, rule->round_records, rule->cutoff, profile.get(), lo.get(), nullptr,
                              nullptr, false, (uint8_t *)dev_keep, keep_cap, list.get(), list_cap, med.get(), totals_d.get(), long_len,
                              st, rounds);
    }
    if (rc != TSX_HIP_OK) return rc;
    unsigned long long h[NT_N] = {0, 0, 0};
    HIP_TRY(hipMemcpyAsync(h, totals_d.get(), sizeof h, hipMemcpyDeviceToHost, st));
    TSX_TRY(normalize_tiles_end(m, nb, st));   // (waits)
    tot.records = nrec; tot.kept = h[NT_KEPT]; tot.kmers_seen = h[NT_SEEN]; tot.kmers_added = h[NT_ADDED]; tot.rounds = rounds;
    if (totals) *totals = tot;
    return nrec > keep_cap && dev_keep ? TSX_HIP_ERANGE : TSX_HIP_OK;
}

// ---- table sizing: the HyperLogLog sketch of a text's k-mers, its estimate, the l that holds them (tsx_sketch.h) --
static bool sketch_prec_ok(int precision) { return precision >= SKETCH_P_MIN && precision <= SKETCH_P_MAX; }

// sketch_windows_kernel over the start positions [0, own_end) of d_text (n readable bytes), after line_pass.
static int sketch_launch(tsx_hip_map *m, const uint8_t *d_text, uint64_t n, uint64_t own_end, int head_open,
                         const unsigned long long *d_line_base, int precision, uint32_t *d_regs, unsigned long long *d_kmers,
                         hipStream_t st) {
    if (own_end == 0) return TSX_HIP_OK;
    const uint64_t ntiles = (own_end + TILE - 1) / TILE;
    const size_t lds = (size_t)4 << precision;   // the workgroup's registers: two workgroups of 64 KiB + 3 KiB fit a CU's 160 KiB
    const int grid = (int)std::min<uint64_t>(ntiles, (uint64_t)m->cus * 2);   // persistent: the fold is bounded by the grid
    hipError_t attr = hipSuccess;
    DISPATCH_BR(m, DISPATCH_CANON(m, DISPATCH_WK(m, {
        auto kern = (sketch_windows_kernel<WKV, CANV, BRV>);
        attr = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (attr == hipSuccess)
            hipLaunchKernelGGL(kern, dim3(grid), dim3(NT), lds, st, m->p, d_text, n, own_end, head_open,
                               (const uint32_t *)m->d_tile.get(), ntiles, d_line_base, precision, d_regs, d_kmers, m->qmap_cur);
    })));
    HIP_TRY(attr);
    HIP_TRY(hipGetLastError());
    return TSX_HIP_OK;
}

extern "C" int tsx_hip_sketch_device(tsx_hip_map *m, const void *dev_text, size_t n, int precision, void *dev_regs,
                                     void *dev_totals, void *stream) {
    if (!m || !dev_regs || !sketch_prec_ok(precision) || (!dev_text && n) || ((uintptr_t)dev_text & 15) ||
        ((uintptr_t)dev_regs & 3) || ((uintptr_t)dev_totals & 7))
        return TSX_HIP_EINVAL;
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t st = pick_stream(m, stream);
    TSX_TRY(base_rule_ok(m));
    const uint8_t *base = (const uint8_t *)dev_text;
    unsigned long long *tot = (unsigned long long *)dev_totals;
    unsigned long long *kmers = tot ? tot : (unsigned long long *)m->d_carry.get() + 4;   // (a word of the scratch nobody reads)
    TSX_TRY(device_windows(m, base, n, false, st,
                           [&](size_t off, size_t own, size_t len, int head_open, bool, const unsigned long long *d_base) {
                               return sketch_launch(m, base + off, len, own, head_open, d_base, precision, (uint32_t *)dev_regs,
                                                    kmers, st);
                           }));
    if (tot) hipLaunchKernelGGL(sketch_records_kernel, dim3(1), dim3(64), 0, st, (const unsigned long long *)m->d_carry.get() + 3, tot);
    HIP_TRY(hipGetLastError());
    return TSX_HIP_OK;
}

// Scratch of one sketch call that works on pieces: the registers and {kmers, records} on the device, their pinned copy.
struct SketchBufs {
    DevBuf<uint32_t> regs;
    DevBuf<unsigned long long> tot;
    PinBuf<uint32_t> h_regs;             // the registers, then the two totals
    PieceBufs p;
    explicit SketchBufs(hipStream_t s) : p(s) {}
    int init(int precision) {
        const size_t nreg = (size_t)1 << precision;
        TSX_TRY(regs.alloc(nreg * sizeof(uint32_t)));
        TSX_TRY(tot.alloc(2 * sizeof(unsigned long long)));
        TSX_TRY(h_regs.alloc(nreg * sizeof(uint32_t) + 2 * sizeof(unsigned long long)));
        HIP_TRY(hipMemsetAsync(regs.get(), 0, nreg * sizeof(uint32_t), p.st));
        HIP_TRY(hipMemsetAsync(tot.get(), 0, 2 * sizeof(unsigned long long), p.st));
        return TSX_HIP_OK;
    }
    // After the last piece: the registers come back once and are max-combined into the caller's, the totals added.
    int collect(int precision, uint8_t *out, tsx_hip_sketch_totals *totals, uint64_t records) {
        const size_t nreg = (size_t)1 << precision;
        unsigned long long *h_tot = (unsigned long long *)(h_regs.get() + nreg);
        HIP_TRY(hipMemcpyAsync(h_regs.get(), regs.get(), nreg * sizeof(uint32_t), hipMemcpyDeviceToHost, p.st));
        HIP_TRY(hipMemcpyAsync(h_tot, tot.get(), sizeof(unsigned long long), hipMemcpyDeviceToHost, p.st));
        HIP_TRY(hipStreamSynchronize(p.st));
        for (size_t i = 0; i < nreg; ++i) out[i] = (uint8_t)std::max<uint32_t>(out[i], h_regs.get()[i]);
        if (totals) { totals->kmers += h_tot[0]; totals->records += records; }
        return TSX_HIP_OK;
    }
};

// One piece: piece_front, then the sketch of its whole records [0, cut), queued and not waited for.  Not last and no
// whole record: nrec = 0, nothing done.
static int sketch_piece(tsx_hip_map *m, SketchBufs &b, const uint8_t *d_text, uint64_t len, bool last, int precision,
                        hipStream_t st, uint64_t &cut, uint64_t &nrec, bool &open) {
    TSX_TRY(piece_front(m, b.p, d_text, len, last, false, cut, nrec, open));
    if (nrec == 0) return TSX_HIP_OK;
    QmapScope qs(m);
    TSX_TRY(piece_qmap(m, d_text, cut, st));
    return sketch_launch(m, d_text, cut, cut, 0, b.p.info.get() + 4, precision, b.regs.get(), b.tot.get(), st);
}

extern "C" int tsx_hip_sketch_host(tsx_hip_map *m, const char *text, size_t n, int precision, uint8_t *regs,
                                   tsx_hip_sketch_totals *totals, size_t chunk_bytes) {
    if (!m || !regs || !sketch_prec_ok(precision) || (!text && n)) return TSX_HIP_EINVAL;
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t st = m->stream.get();
    SketchBufs b(st);
    TSX_TRY(b.init(precision));
    uint64_t rec_base = 0;
    TSX_TRY(host_pieces(m, b.p, text, n, chunk_bytes, true, rec_base,
        [&](const uint8_t *d_text, uint64_t len, bool last, uint64_t &cut, uint64_t &nrec, bool &open) {
            return sketch_piece(m, b, d_text, len, last, precision, st, cut, nrec, open);
        },
        [&](size_t, uint64_t, uint64_t, uint64_t, bool) -> int { return TSX_HIP_OK; }));
    return b.collect(precision, regs, totals, rec_base);
}

// The pieces of bgzf_record_pieces, without a limit on the carried record.
extern "C" int tsx_hip_sketch_bgzf_host(tsx_hip_map *m, const void *gz, size_t n, int precision, uint8_t *regs,
                                        tsx_hip_sketch_totals *totals) {
    if (!m || !regs || !sketch_prec_ok(precision) || (!gz && n)) return TSX_HIP_EINVAL;
    BgzfIndex ix;
    if (!bgzf_index((const uint8_t *)gz, n, ix)) { g_last_error = "not a BGZF file (no BC extra field in every gzip member)"; return TSX_HIP_EINVAL; }
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t st = m->stream.get();
    join_foreign(m, false);
    TSX_TRY(base_rule_ok(m));
    SketchBufs b(st);
    TSX_TRY(b.init(precision));
    TSX_TRY(b.p.init());
    uint64_t records = 0;
    TSX_TRY(bgzf_record_pieces((const uint8_t *)gz, n, ix, SIZE_MAX, st, [&](const uint8_t *piece, uint64_t len, bool last, uint64_t &cut) -> int {
        uint64_t nrec = 0;
        bool open = false;
        TSX_TRY(sketch_piece(m, b, piece, len, last, precision, st, cut, nrec, open));
        records += nrec;
        return TSX_HIP_OK;
    }));
    return b.collect(precision, regs, totals, records);
}

template <int WK>
static void sketch_kmers(const uint64_t *kmers, size_t n, uint64_t top, int precision, uint8_t *regs) {
    for (size_t i = 0; i < n; ++i) {
        uint64_t x[WK];
        for (int t = 0; t < WK; ++t) x[t] = kmers[i * WK + t];
        x[WK - 1] &= top;
        uint32_t idx, rank;
        sketch_slot(sketch_hash<WK>(x), precision, idx, rank);
        if (rank > regs[idx]) regs[idx] = (uint8_t)rank;
    }
}

extern "C" int tsx_hip_sketch_kmers_host(int k, const uint64_t *kmers, size_t n, int precision, uint8_t *regs) {
    if (k < 1 || k > 127 || !regs || !sketch_prec_ok(precision) || (!kmers && n)) return TSX_HIP_EINVAL;
    const uint64_t top = ((2 * k) & 63) ? ((1ULL << ((2 * k) & 63)) - 1ULL) : ~0ULL;
    switch ((2 * k + 63) / 64) {
        case 1: sketch_kmers<1>(kmers, n, top, precision, regs); break;
        case 2: sketch_kmers<2>(kmers, n, top, precision, regs); break;
        case 3: sketch_kmers<3>(kmers, n, top, precision, regs); break;
        default: sketch_kmers<4>(kmers, n, top, precision, regs); break;
    }
    return TSX_HIP_OK;
}

extern "C" double tsx_hip_sketch_estimate_host(const uint8_t *regs, int precision) {
    if (!regs || !sketch_prec_ok(precision)) return -1.0;
    const size_t nreg = (size_t)1 << precision;
    const int top = 64 - precision + 1;
    uint64_t hist[66] = {0};
    for (size_t i = 0; i < nreg; ++i) {
        if (regs[i] > top) return -1.0;
        ++hist[regs[i]];
    }
    double sum = 0.0;   // ranks ascending: the order of the Python form
    for (int r = 0; r <= top; ++r) sum += (double)hist[r] * std::ldexp(1.0, -r);
    const double md = (double)nreg, alpha = 0.7213 / (1.0 + 1.079 / md);
    double e = alpha * md * md / sum;
    if (e <= 2.5 * md && hist[0] > 0) e = md * std::log(md / (double)hist[0]);
    return e;
}

extern "C" int tsx_hip_suggest_l(int k, double distinct, int precision, uint32_t load_ppm, int *l_out) {
    if (k < 1 || k > 127 || !l_out || !sketch_prec_ok(precision) || !(distinct >= 0.0) || !std::isfinite(distinct) ||
        load_ppm > 900000u)
        return TSX_HIP_EINVAL;
    const double load = (load_ppm ? load_ppm : 750000u) / 1e6;
    const double need = distinct * (1.0 + 5.0 * 1.04 / std::sqrt((double)((uint64_t)1 << precision))) / load;
    int l = 0;
    while (l < 64 && std::ldexp(1.0, l) < need) ++l;
    l = std::max(4, l);
    const int hi = std::min(36, 2 * k - 1);   // derive_layout's bound and the reference's 2k > l
    if (l > hi) {
        *l_out = hi;
        return distinct / std::ldexp(1.0, hi) > 0.9 ? TSX_HIP_ERANGE : TSX_HIP_OK;
    }
    *l_out = l;
    return TSX_HIP_OK;
}

// ---- counting only the k-mers seen twice: the prefilter of a map, its two passes (tsx_prefilter.h) -------------------
static bool prefilter_bits_ok(int bits) { return bits >= PF_BITS_MIN && bits <= PF_BITS_MAX; }
static inline size_t pf_words_a(int bits) { return (size_t)1 << (bits - 6); }
static inline size_t pf_words_b(int bits) { return (size_t)1 << (bits - 8); }

extern "C" int tsx_hip_prefilter_create(tsx_hip_map *m, int bits) {
    if (!m || !prefilter_bits_ok(bits)) return TSX_HIP_EINVAL;
    HIP_TRY(hipSetDevice(m->device));
    join_foreign(m, false);
    hipStream_t st = m->stream.get();
    HIP_TRY(hipStreamSynchronize(st));   // (filters that are replaced may still be read)
    m->pf_bits = 0; m->pf_armed = false;
    int rc = m->pf_a.alloc(pf_words_a(bits) * 8);
    if (rc == TSX_HIP_OK) rc = m->pf_b.alloc(pf_words_b(bits) * 8);
    if (rc == TSX_HIP_OK && !m->pf_tot.get()) rc = m->pf_tot.alloc(PF_NTOT * sizeof(unsigned long long));
    if (rc == TSX_HIP_OK && !m->pf_ev.get()) rc = m->pf_ev.create();
    if (rc != TSX_HIP_OK) { m->pf_a.reset(); m->pf_b.reset(); return rc; }
    HIP_TRY(hipMemsetAsync(m->pf_a.get(), 0, pf_words_a(bits) * 8, st));
    HIP_TRY(hipMemsetAsync(m->pf_b.get(), 0, pf_words_b(bits) * 8, st));
    HIP_TRY(hipMemsetAsync(m->pf_tot.get(), 0, PF_NTOT * sizeof(unsigned long long), st));
    // waited for: pass 1 may come on a caller's stream, which nothing else orders behind this one (creating is not hot)
    HIP_TRY(hipStreamSynchronize(st));
    m->pf_bits = bits;
    return TSX_HIP_OK;
}

extern "C" int tsx_hip_prefilter_free(tsx_hip_map *m) {
    if (!m) return TSX_HIP_EINVAL;
    if (!m->pf_bits) return TSX_HIP_OK;
    HIP_TRY(hipSetDevice(m->device));
    join_foreign(m, true);
    HIP_TRY(hipStreamSynchronize(m->stream.get()));
    m->pf_bits = 0; m->pf_armed = false;
    m->pf_a.reset(); m->pf_b.reset();
    return TSX_HIP_OK;
}

extern "C" int tsx_hip_prefilter_arm(tsx_hip_map *m, int on) {
    if (!m || (on && !m->pf_bits)) return TSX_HIP_EINVAL;
    m->pf_armed = on != 0;
    return TSX_HIP_OK;
}

extern "C" int tsx_hip_prefilter_bits(const tsx_hip_map *m) {
    if (!m) return TSX_HIP_EINVAL;
    return m->pf_bits;
}

extern "C" int tsx_hip_prefilter_armed(const tsx_hip_map *m) {
    if (!m) return TSX_HIP_EINVAL;
    return m->pf_armed ? 1 : 0;
}

// prefilter_windows_kernel over the start positions [0, own_end) of d_text (n readable bytes), after line_pass.
static int prefilter_launch(tsx_hip_map *m, const uint8_t *d_text, uint64_t n, uint64_t own_end, int head_open,
                            const unsigned long long *d_line_base, hipStream_t st) {
    if (own_end == 0) return TSX_HIP_OK;
    const uint64_t ntiles = (own_end + TILE - 1) / TILE;
    const int grid = (int)std::min<uint64_t>(ntiles, (uint64_t)m->cus * 8);
    DISPATCH_BR(m, DISPATCH_CANON(m, DISPATCH_WK(m, hipLaunchKernelGGL((prefilter_windows_kernel<WKV, CANV, BRV>), dim3(grid), dim3(NT), 0,
                                                        st, m->p, d_text, n, own_end, head_open, (const uint32_t *)m->d_tile.get(),
                                                        ntiles, d_line_base, m->pf_bits, m->pf_a.get(), m->pf_b.get(),
                                                        m->pf_tot.get(), m->qmap_cur))));
    HIP_TRY(hipGetLastError());
    return TSX_HIP_OK;
}

// One piece: piece_front, then pass 1 over its whole records [0, cut), queued and not waited for.  Not last and no
// whole record: nrec = 0, nothing done.
static int prefilter_piece(tsx_hip_map *m, PieceBufs &p, const uint8_t *d_text, uint64_t len, bool last, hipStream_t st,
                           uint64_t &cut, uint64_t &nrec, bool &open) {
    TSX_TRY(piece_front(m, p, d_text, len, last, false, cut, nrec, open));
    if (nrec == 0) return TSX_HIP_OK;
    QmapScope qs(m);
    TSX_TRY(piece_qmap(m, d_text, cut, st));
    return prefilter_launch(m, d_text, cut, cut, 0, p.info.get() + 4, st);
}

extern "C" int tsx_hip_prefilter_add_host(tsx_hip_map *m, const char *text, size_t n, size_t chunk_bytes) {
    if (!m || !m->pf_bits || (!text && n)) return TSX_HIP_EINVAL;
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t st = m->stream.get();
    PieceBufs p(st);
    uint64_t rec_base = 0;
    return host_pieces(m, p, text, n, chunk_bytes, true, rec_base,
        [&](const uint8_t *d_text, uint64_t len, bool last, uint64_t &cut, uint64_t &nrec, bool &open) {
            return prefilter_piece(m, p, d_text, len, last, st, cut, nrec, open);
        },
        [&](size_t, uint64_t, uint64_t, uint64_t, bool) -> int { return TSX_HIP_OK; });
}

// The pieces of bgzf_record_pieces, without a limit on the carried record.
extern "C" int tsx_hip_prefilter_add_bgzf_host(tsx_hip_map *m, const void *gz, size_t n) {
    if (!m || !m->pf_bits || (!gz && n)) return TSX_HIP_EINVAL;
    BgzfIndex ix;
    if (!bgzf_index((const uint8_t *)gz, n, ix)) { g_last_error = "not a BGZF file (no BC extra field in every gzip member)"; return TSX_HIP_EINVAL; }
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t st = m->stream.get();
    join_foreign(m, false);
    TSX_TRY(base_rule_ok(m));
    PieceBufs p(st);
    TSX_TRY(p.init());
    return bgzf_record_pieces((const uint8_t *)gz, n, ix, SIZE_MAX, st, [&](const uint8_t *piece, uint64_t len, bool last, uint64_t &cut) -> int {
        uint64_t nrec = 0;
        bool open = false;
        return prefilter_piece(m, p, piece, len, last, st, cut, nrec, open);
    });
}

extern "C" int tsx_hip_prefilter_add_device(tsx_hip_map *m, const void *dev_text, size_t n, void *stream) {
    if (!m || !m->pf_bits || (!dev_text && n) || ((uintptr_t)dev_text & 15)) return TSX_HIP_EINVAL;
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t st = pick_stream(m, stream);
    TSX_TRY(base_rule_ok(m));
    const uint8_t *base = (const uint8_t *)dev_text;
    return device_windows(m, base, n, false, st,
                          [&](size_t off, size_t own, size_t len, int head_open, bool, const unsigned long long *d_base) {
                              return prefilter_launch(m, base + off, len, own, head_open, d_base, st);
                          });
}

extern "C" int tsx_hip_prefilter_stats(tsx_hip_map *m, tsx_hip_prefilter_totals *out) {
    if (!m || !out) return TSX_HIP_EINVAL;
    memset(out, 0, sizeof *out);
    if (!m->pf_bits) return TSX_HIP_OK;
    HIP_TRY(hipSetDevice(m->device));
    join_foreign(m, true);
    hipStream_t st = m->stream.get();
    unsigned long long *tot = m->pf_tot.get();
    HIP_TRY(hipMemsetAsync(tot + PF_SET_A, 0, 2 * sizeof(unsigned long long), st));
    const uint64_t na = pf_words_a(m->pf_bits), nb = pf_words_b(m->pf_bits);
    hipLaunchKernelGGL(prefilter_fill_kernel, dim3(grid_for(m, na, 8)), dim3(NT), 0, st, (const unsigned long long *)m->pf_a.get(), na,
                       (const unsigned long long *)m->pf_b.get(), nb, tot);
    HIP_TRY(hipGetLastError());
    unsigned long long h[PF_NTOT];
    HIP_TRY(hipMemcpyAsync(h, tot, sizeof h, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    out->bits = (uint64_t)m->pf_bits;
    out->seen = h[PF_SEEN]; out->seen_again = h[PF_AGAIN]; out->admitted = h[PF_ADMITTED]; out->skipped = h[PF_SKIPPED];
    out->set_bits_a = h[PF_SET_A]; out->set_bits_b = h[PF_SET_B];
    return TSX_HIP_OK;
}

extern "C" int tsx_hip_prefilter_read(tsx_hip_map *m, int which, uint64_t *words_out, size_t nwords) {
    if (!m || !m->pf_bits || which < 0 || which > 1 || (!words_out && nwords)) return TSX_HIP_EINVAL;
    const size_t have = which ? pf_words_b(m->pf_bits) : pf_words_a(m->pf_bits);
    if (nwords != have) return TSX_HIP_ERANGE;
    HIP_TRY(hipSetDevice(m->device));
    join_foreign(m, true);
    HIP_TRY(hipMemcpyAsync(words_out, which ? m->pf_b.get() : m->pf_a.get(), have * 8, hipMemcpyDeviceToHost, m->stream.get()));
    HIP_TRY(hipStreamSynchronize(m->stream.get()));
    return TSX_HIP_OK;
}

template <int WK>
static void prefilter_mask_of(const uint64_t *kmer, uint64_t top, int bits, uint64_t *word_a, uint64_t *word_b, uint64_t *mask) {
    uint64_t x[WK];
    for (int t = 0; t < WK; ++t) x[t] = kmer[t];
    x[WK - 1] &= top;
    const uint64_t v = sketch_hash<WK>(x);
    if (word_a) *word_a = pf_word_a(v, bits);
    if (word_b) *word_b = pf_word_b(v, bits);
    if (mask) *mask = pf_mask(v);
}

extern "C" int tsx_hip_prefilter_mask_host(int k, const uint64_t *kmer_limbs, int bits, uint64_t *word_a, uint64_t *word_b,
                                           uint64_t *mask) {
    if (k < 1 || k > 127 || !kmer_limbs || !prefilter_bits_ok(bits)) return TSX_HIP_EINVAL;
    const uint64_t top = ((2 * k) & 63) ? ((1ULL << ((2 * k) & 63)) - 1ULL) : ~0ULL;
    switch ((2 * k + 63) / 64) {
        case 1: prefilter_mask_of<1>(kmer_limbs, top, bits, word_a, word_b, mask); break;
        case 2: prefilter_mask_of<2>(kmer_limbs, top, bits, word_a, word_b, mask); break;
        case 3: prefilter_mask_of<3>(kmer_limbs, top, bits, word_a, word_b, mask); break;
        default: prefilter_mask_of<4>(kmer_limbs, top, bits, word_a, word_b, mask); break;
    }
    return TSX_HIP_OK;
}

// ---- paired reads: the filter and the trim over mate pairs (tsx_pairs.h) -----------------------------------------
// One input text of a pair call: where the next piece starts, and the scratch of the single-end path that works on it
// (q for the filter, t for the trim; p is the piece scratch of the one in use, the only one initialised).
struct PairSide {
    QueryBufs q;
    TrimBufs t;
    PieceBufs &p;
    const char *text = nullptr;
    size_t n = 0, off = 0, len = 0;
    bool last = false;
    PairSide(hipStream_t st, bool trim) : q(st), t(st), p(trim ? t.p : q.p) {}
};
static int pair_fail(const std::string &what) { g_last_error = what; return TSX_HIP_EPAIR; }

// One pair call (trule: the trim, else frule: the filter).  Outputs: 0 kept mates 1, 1 kept mates 2, 2 orphans of A,
// 3 orphans of B; an interleaved text (text2 == NULL) uses 0 and 2 for both mates.  Every round: a piece of each text,
// both scans, pair_cut_kernel and ONE wait for the record count R and the cuts; then records [0, R) of each piece through
// the single-end kernels, the gate, one compaction per output.  The outputs of round i are written while the device
// works on round i + 1.  One method per step of a round; run() is the rounds, finish() every way out.
struct PairRun {
    tsx_hip_map *m;
    hipStream_t st;
    const tsx_hip_filter_rule *frule;
    const tsx_hip_trim_rule *trule;
    int any, check_names;
    size_t chunk_bytes;
    bool trim, inter;
    int ns;                     // texts
    uint32_t stride, per;       // records of a text per pair; entries of a length array per record
    tsx_hip_pair_totals t;
    uint64_t R = 0, cut[2] = {0, 0};      // what the round agreed on: the records it takes of each piece, where the pieces end
    bool open[2] = {false, false};
    WriteBehind wb[4];          // (fd < 0: not wanted, or not used)
    Compaction out[4];          // the gated lengths of an output (scanned in place) and its bytes
    DevBuf<unsigned long long> pinfo;
    PinBuf<unsigned long long> h_pinfo;
    Event ev;
    PairSide side[2];   // (the sides are declared last: their destructors wait for the stream before anything above is released)

    PairRun(tsx_hip_map *mm, const tsx_hip_filter_rule *fr, const tsx_hip_trim_rule *tr, int any_, int names, size_t chunk, bool inter_)
        : m(mm), st(mm->stream.get()), frule(fr), trule(tr), any(any_), check_names(names), chunk_bytes(chunk), trim(tr != nullptr),
          inter(inter_), ns(inter_ ? 1 : 2), stride(inter_ ? 2u : 1u), per(tr ? 4u : 1u),
          side{PairSide(mm->stream.get(), tr != nullptr), PairSide(mm->stream.get(), tr != nullptr)} {
        memset(&t, 0, sizeof t);
    }
    bool used(int oi) const { return !inter || !(oi & 1); }   // the gate writes its lengths
    int init(const char *text1, size_t n1, const char *text2, size_t n2, const tsx_hip_pair_io &io) {
        side[0].text = text1; side[0].n = n1;
        side[1].text = text2; side[1].n = inter ? 0 : n2;
        const int fd[4] = {io.fd1, io.fd2, io.fd_single1, io.fd_single2};
        for (int oi = 0; oi < 4; ++oi) wb[oi].fd = used(oi) ? fd[oi] : -1;
        for (int i = 0; i < ns; ++i) TSX_TRY(side[i].p.init());
        TSX_TRY(pinfo.alloc(PI_N * sizeof(unsigned long long)));
        HIP_TRY(hipMemsetAsync(pinfo.get(), 0, PI_N * sizeof(unsigned long long), st));
        TSX_TRY(h_pinfo.alloc(PI_N * sizeof(unsigned long long)));
        return ev.create();
    }
    // The piece [off, off + len) of a side to the device, and its scan (an empty piece: no records).
    int scan(PairSide &s) {
        s.last = s.off + s.len == s.n;
        if (s.len == 0) {
            HIP_TRY(hipMemsetAsync(s.p.info.get(), 0, 3 * sizeof(unsigned long long), st));
            return TSX_HIP_OK;
        }
        TSX_TRY(piece_upload(s.p, s.text + s.off, s.len));
        return piece_scan(m, s.p.text.get(), s.len, s.last, s.p.info.get(), &s.p.rspan, st);
    }
    int longer(PairSide &s) {   // a piece without a whole record (interleaved: a whole pair) grows
        TSX_TRY(piece_longer(s.len, s.n - s.off));
        return scan(s);
    }

    // The cut: pair_cut_kernel and the one wait of a round, again while a side that holds no whole record (pair) can
    // grow.  done: nothing but empty lines is left.  Texts that are out of step: TSX_HIP_EPAIR.
    int agree(bool &done) {
        const unsigned long long *h = h_pinfo.get();
        for (bool again = true; again;) {
            hipLaunchKernelGGL(pair_cut_kernel, dim3(1), dim3(64), 0, st, (const unsigned long long *)side[0].p.info.get(),
                               (const unsigned long long *)side[0].p.rspan.get(),
                               inter ? (const unsigned long long *)nullptr : (const unsigned long long *)side[1].p.info.get(),
                               inter ? (const unsigned long long *)nullptr : (const unsigned long long *)side[1].p.rspan.get(),
                               side[0].last ? 1 : 0, pinfo.get());
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(h_pinfo.get(), pinfo.get(), 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            again = false;
            if (h[inter ? PI_R : PI_RA] == 0 && !side[0].last) { TSX_TRY(longer(side[0])); again = true; }
            if (!inter && h[PI_RB] == 0 && !side[1].last) { TSX_TRY(longer(side[1])); again = true; }
        }
        const uint64_t RA = h[PI_RA], RB = h[PI_RB];
        R = h[PI_R];
        cut[0] = h[PI_CUT_A]; cut[1] = h[PI_CUT_B];
        open[0] = h[PI_OPEN_A] != 0; open[1] = h[PI_OPEN_B] != 0;
        if (inter) {
            if (side[0].last && (RA & 1))
                return pair_fail("an interleaved text with an odd number of records (" + std::to_string(2 * t.pairs + RA) + ")");
            done = R == 0;   // (nothing but empty lines)
            return TSX_HIP_OK;
        }
        done = RA == 0 && RB == 0;   // (nothing but empty lines in either)
        if (!done && R == 0)
            return pair_fail(std::string("text ") + (RA ? "2" : "1") + " ends after " + std::to_string(t.pairs) +
                             " records, text " + (RA ? "1" : "2") + " holds more");
        return TSX_HIP_OK;
    }

    // Records [0, R) of each piece through the single-end kernels (the line pass again: the tile counts are the map's, and
    // the other text's by now).
    int records() {
        for (int i = 0; i < ns; ++i) {
            PairSide &s = side[i];
            const uint8_t *d_text = s.p.text.get();
            HIP_TRY(hipMemsetAsync(m->d_carry.get(), 0, sizeof(uint32_t), st));
            TSX_TRY(line_pass(m, d_text, cut[i], cut[i], 0, st));
            if (trim) {
                TSX_TRY(trim_records(m, s.t, d_text, cut[i], R, s.last && cut[i] == s.len, *trule, st));
                TSX_TRY(trim_lens(m, s.t, R, *trule, pinfo.get() + (i ? PI_TRIM_B : PI_TRIM_A), st));
            } else {
                TSX_TRY(query_records(m, s.q, d_text, cut[i], R, frule->lower, frule->upper, st));
            }
        }
        return TSX_HIP_OK;
    }

    // The names, and the gate: what each mate gives to every output that is used.  An interleaved text keeps both mates'
    // lengths in one array: mate 2's entries are mate 1's moved on by one record.
    int gate() {
        const uint64_t npairs = R / stride, ne = R * per;
        unsigned long long *const pi = pinfo.get(), *len[4] = {nullptr, nullptr, nullptr, nullptr};
        for (int oi = 0; oi < 4; ++oi)
            if (used(oi)) TSX_TRY(out[oi].lengths(st, ne, len[oi]));
        PairSide &sb = side[inter ? 0 : 1];   // where mate 2 lives
        unsigned long long *const keep_a = len[0], *const single_a = len[2];
        unsigned long long *const keep_b = inter ? keep_a + per : len[1];
        unsigned long long *const single_b = inter ? single_a + per : len[3];
        const unsigned long long *span_a = side[0].p.rspan.get(), *span_b = inter ? span_a + 2 : side[1].p.rspan.get();
        if (check_names)
            hipLaunchKernelGGL(pair_names_kernel, dim3(grid_for(m, npairs, 8)), dim3(NT), 0, st, (const uint8_t *)side[0].p.text.get(),
                               span_a, (const uint8_t *)sb.p.text.get(), span_b, npairs, stride, pi + PI_BAD);
        if (trim) {
            const unsigned long long *seg_a = side[0].t.c.off.get(), *seg_b = inter ? seg_a + 4 : side[1].t.c.off.get();
            hipLaunchKernelGGL(pair_gate_trim_kernel, dim3(grid_for(m, npairs, 8)), dim3(NT), 0, st, seg_a, seg_b, npairs, stride,
                               keep_a, keep_b, single_a, single_b, pi + PI_KEPT);
        } else {
            const unsigned long long *st_a = side[0].q.stats.get(), *st_b = inter ? st_a + QS_N : side[1].q.stats.get();
            hipLaunchKernelGGL(pair_gate_filter_kernel, dim3(grid_for(m, npairs, 8)), dim3(NT), 0, st, st_a, span_a, st_b, span_b,
                               npairs, stride, frule->min_in_range, (uint64_t)frule->fraction_ppm, frule->invert, any,
                               (!inter && open[0]) ? 1 : 0, (inter ? open[0] : open[1]) ? 1 : 0, keep_a, keep_b, single_a, single_b,
                               pi + PI_KEPT);
        }
        HIP_TRY(hipGetLastError());
        return TSX_HIP_OK;
    }

    // One compaction per wanted output, out of the text its mates live in; the sizes go to pinfo[PI_TOTAL ..].
    int compact() {
        const uint64_t ne = R * per;
        for (int oi = 0; oi < 4; ++oi) {
            if (wb[oi].fd < 0) continue;
            const int si = inter ? 0 : (oi & 1);
            PairSide &s = side[si];
            unsigned long long *total = pinfo.get() + PI_TOTAL + oi;
            if (trim) TSX_TRY(out[oi].copy_segments(m, s.p.text.get(), cut[si], s.t.src.get(), ne, total, st));
            else TSX_TRY(out[oi].copy_spans(m, s.p.text.get(), cut[si], s.p.rspan.get(), ne, total, st));
        }
        return TSX_HIP_OK;
    }

    // The write-behind round.  The names are looked at between its two steps: a round with a bad pair stages nothing.
    int deliver() {
        const unsigned long long *h = h_pinfo.get();
        TSX_TRY(WriteBehind::words_back(wb, 4, pinfo.get(), h_pinfo.get(), PI_N, ev.get(), st));
        if (h[PI_BAD]) return pair_fail("pair " + std::to_string(t.pairs + (uint64_t)~h[PI_BAD]) + ": the names of the mates differ");
        const uint8_t *d_out[4];
        uint64_t cuts[4];
        for (int oi = 0; oi < 4; ++oi) { d_out[oi] = out[oi].out.out; cuts[oi] = cut[inter ? 0 : (oi & 1)]; }
        // (the counters are per round)
        TSX_TRY(WriteBehind::stage_all(wb, 4, d_out, h + PI_TOTAL, cuts, "pair", pinfo.get() + PI_KEPT, PI_N - PI_KEPT, st));
        t.pairs += R / stride; t.kept += h[PI_KEPT]; t.single1 += h[PI_SINGLE_A]; t.single2 += h[PI_SINGLE_B];
        t.bases_in += h[PI_TRIM_A + 1] + h[PI_TRIM_B + 1];
        t.bases_kept += h[PI_TRIM_A + 2] + h[PI_TRIM_B + 2];
        for (int i = 0; i < ns; ++i) side[i].off += cut[i];
        return TSX_HIP_OK;
    }

    int run() {
        for (;;) {
            bool rest = false, done = false;
            for (int i = 0; i < ns; ++i) rest |= side[i].off < side[i].n;
            if (!rest) return TSX_HIP_OK;
            for (int i = 0; i < ns; ++i) {
                side[i].len = std::min(chunk_bytes, side[i].n - side[i].off);
                TSX_TRY(scan(side[i]));
            }
            TSX_TRY(agree(done));
            if (done) return TSX_HIP_OK;
            TSX_TRY(records());
            TSX_TRY(gate());
            TSX_TRY(compact());
            TSX_TRY(deliver());
        }
    }

    // Every way out: the totals; and what waits goes to its files after TSX_HIP_EPAIR too -- whole pairs of the rounds
    // before the one that failed -- with the error's text kept.
    int finish(int rc, tsx_hip_pair_totals *totals) {
        const std::string why = g_last_error;
        for (WriteBehind &w : wb)
            if (rc == TSX_HIP_OK || rc == TSX_HIP_EPAIR) { const int wrc = w.flush(); if (wrc != TSX_HIP_OK) rc = wrc; }
        if (rc == TSX_HIP_OK || rc == TSX_HIP_EPAIR) g_last_error = why;
        t.bytes1 = wb[0].bytes; t.bytes2 = wb[1].bytes; t.bytes_single1 = wb[2].bytes; t.bytes_single2 = wb[3].bytes;
        if (totals) *totals = t;
        return rc;
    }
};

static int pairs_host(tsx_hip_map *m, const char *text1, size_t n1, const char *text2, size_t n2, const tsx_hip_filter_rule *frule,
                      const tsx_hip_trim_rule *trule, int any, int check_names, const tsx_hip_pair_io &io, size_t chunk_bytes,
                      tsx_hip_pair_totals *totals) {
    TSX_TRY(pieces_begin(m, chunk_bytes, false));   // (ahead of the run: a call refused here has built and waited for nothing)
    PairRun run(m, frule, trule, any, check_names, chunk_bytes, text2 == nullptr);
    const int rc = run.init(text1, n1, text2, n2, io);
    return run.finish(rc == TSX_HIP_OK ? run.run() : rc, totals);
}

static bool pair_io_ok(const tsx_hip_pair_io *io, bool inter) {
    if (!io || io->fd1 < 0) return false;
    return inter ? (io->fd2 == -1 && io->fd_single2 == -1) : io->fd2 >= 0;
}

extern "C" int tsx_hip_filter_pairs_host(tsx_hip_map *m, const char *text1, size_t n1, const char *text2, size_t n2,
                                         const tsx_hip_filter_rule *rule, int pair_mode, int check_names, const tsx_hip_pair_io *io,
                                         size_t chunk_bytes, tsx_hip_pair_totals *totals) {
    if (totals) memset(totals, 0, sizeof *totals);
    if (!rule_ok(rule) || !query_args_ok(m, rule->lower, rule->upper) || (!text1 && n1) || (!text2 && n2) ||
        (pair_mode != TSX_HIP_PAIR_BOTH && pair_mode != TSX_HIP_PAIR_ANY) || !pair_io_ok(io, text2 == nullptr))
        return TSX_HIP_EINVAL;
    return pairs_host(m, text1, n1, text2, n2, rule, nullptr, pair_mode == TSX_HIP_PAIR_ANY ? 1 : 0, check_names, *io, chunk_bytes, totals);
}

extern "C" int tsx_hip_trim_pairs_host(tsx_hip_map *m, const char *text1, size_t n1, const char *text2, size_t n2,
                                       const tsx_hip_trim_rule *rule, int check_names, const tsx_hip_pair_io *io, size_t chunk_bytes,
                                       tsx_hip_pair_totals *totals) {
    if (totals) memset(totals, 0, sizeof *totals);
    if (!trim_rule_ok(m, rule) || (!text1 && n1) || (!text2 && n2) || !pair_io_ok(io, text2 == nullptr)) return TSX_HIP_EINVAL;
    return pairs_host(m, text1, n1, text2, n2, nullptr, rule, 0, check_names, *io, chunk_bytes, totals);
}
