/*
 * tsxcount_hip.h -- C ABI of libtsxcount_hip.so, the MI355X (gfx950) k-mer
 * counting hash map that backs tsxCount's --mode=HIP.
 *
 * Every entry point is what a TSXHashMap subclass in the reference would bind
 * for this path; the reference interface each one replaces is cited as
 * file:line of mjoppich/tsxCount.  Plain pointers and sizes only.  All
 * functions return TSX_HIP_OK (0) or a negative TSX_HIP_E* code; none of them
 * falls back to a CPU path -- without a GPU they fail with TSX_HIP_ENODEVICE.
 *
 * k-mers cross the boundary 2-bit encoded exactly like UBigInt holds them in
 * the reference (src/utils/SequenceUtils.h:86-160): base i of the k-mer sits
 * in bits 2i,2i+1 (A=0 C=1 G=2 T=3), packed little-endian into
 * tsx_hip_key_limbs(k) = ceil(2k/64) uint64 limbs per k-mer.
 */
#ifndef TSXCOUNT_HIP_H
#define TSXCOUNT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tsx_hip_map tsx_hip_map; /* opaque: one table on one GPU */

enum {
    TSX_HIP_OK = 0,
    TSX_HIP_EINVAL = -1,    /* bad argument; 2k <= l mirrors TSXException (TSXHashMap.h:91-94) */
    TSX_HIP_ENODEVICE = -2, /* no usable HIP device */
    TSX_HIP_ENOMEM = -3,    /* device allocation failed */
    TSX_HIP_EHIP = -4,      /* a HIP runtime call failed (see tsx_hip_last_error) */
    TSX_HIP_EFULL = -5,     /* a k-mer could not be placed: reference exit(42), TSXHashMap.h:340-343 */
    TSX_HIP_EOVERFLOW = -6, /* the secondary (count overflow) array is full */
    TSX_HIP_ERANGE = -7,    /* output buffer too small */
    TSX_HIP_ELOCK = -8,     /* a multi-limb slot stayed locked past the spin bound: counts may be wrong */
    TSX_HIP_EIO = -9,       /* writing an output file failed (see tsx_hip_last_error) */
    TSX_HIP_EFORMAT = -10,  /* not a k-mer database, or a damaged one (see tsx_hip_last_error) */
    TSX_HIP_EPAIR = -11     /* the mates of paired reads do not line up (see tsx_hip_last_error) */
};

/* Layout the library derived from (k, l, storagebits); see DESIGN.md. */
typedef struct tsx_hip_layout {
    int32_t k, l;           /* as given */
    int32_t key_limbs;      /* ceil(2k/64): limbs per k-mer at the boundary */
    int32_t entry_limbs;    /* uint64 limbs per table slot */
    int32_t func_bits;      /* 2k-l hashed-key bits stored in the slot (TSXTypes.h:39) */
    int32_t reprobe_bits;   /* width of the reprobe field stored next to them */
    int32_t count_bits;     /* in-slot counter width ("storage bits", TSXHashMap.h:83) */
    int32_t overflow_l;     /* log2 slots of the secondary overflow array */
    int32_t shard_bits;     /* the whole table has 2^(l+shard_bits) slots spread over 2^shard_bits GPUs */
    int32_t shard_index;    /* this GPU holds home slots [shard_index << l, (shard_index+1) << l) */
    uint32_t max_reprobes;  /* probes tried before TSX_HIP_EFULL */
    uint64_t slots;         /* 2^l (getMaxElements, TSXHashMap.h:162) */
    uint64_t table_bytes;   /* device bytes of the primary table */
} tsx_hip_layout;

/* Counters kept on the device; print_stats()/main.cpp:479-501 equivalents. */
typedef struct tsx_hip_stats {
    uint64_t kmers_added;      /* k-mer occurrences inserted ("add calls") */
    uint64_t insert_failures;  /* occurrences lost to TSX_HIP_EFULL */
    uint64_t overflow_carries; /* carries pushed to the secondary array */
    uint64_t overflow_failures;/* carries lost to TSX_HIP_EOVERFLOW */
    uint64_t distinct;         /* occupied slots = getKmerCount() (TSXHashMap.h:645) */
    uint64_t overflow_used;    /* occupied secondary slots */
    uint64_t lock_timeouts;    /* multi-limb claim spins that gave up (must be 0) */
    uint64_t fallback_inserts; /* keys the partitioned path inserted atomically because a list was full */
    uint64_t count_sum;        /* sum of getKmerCount(kmer) over every stored k-mer, read back from the slots
                                  and the secondary array: equals kmers_added when nothing was lost (the
                                  reference's --check walks every k-mer instead, main.cpp:224-396) */
} tsx_hip_stats;

int tsx_hip_key_limbs(int k);
const char *tsx_hip_strerror(int code);
const char *tsx_hip_last_error(void); /* text of the last HIP runtime failure in this thread */
int tsx_hip_device_count(void);

/* TSXSeqUtils::fromSequence (SequenceUtils.h:86-160).  Non-ACGT bytes get the
 * fixed code ((b>>1)^(b>>2))&3 where the reference draws rand()%2 bits.      */
int tsx_hip_encode(const char *seq, int k, uint64_t *limbs_out);
/* TSXSeqUtils::toSequence (SequenceUtils.h:47-84). out must hold k+1 bytes. */
int tsx_hip_decode(const uint64_t *limbs, int k, char *out);

/*
 * TSXHashMap(iL, iStorageBits, iK) (TSXHashMap.h:79-154) and
 * TSXHashMapCAS(iL, iStorageBits, iK, iThreads) (TSXHashMapCAS.h:239-245).
 *   storagebits  0 = widest counter that fits the slot; 1..32 = exactly that
 *                many in-slot bits, larger counts carry into the secondary
 *                array (the reference chains overflow slots instead,
 *                TSXHashMapPerf.h:699-881).
 *   overflow_l   log2 slots of the secondary array; 0 = max(10, l-4).
 *   hash_seed    seed of the bijective GF(2) mapping; the reference draws it
 *                from time(NULL) (BijectiveKMapping.h:84).  The matrix is dense:
 *                multiplication by a random element of GF(2^2k), for every k <= 127
 *                (the reference uses a unit triangular matrix, which makes the slot a
 *                function of the first l/2 bases only).
 *   device       HIP device ordinal.
 */
int tsx_hip_create(tsx_hip_map **out, int k, int l, int storagebits, int overflow_l,
                   uint64_t hash_seed, int device);
/*
 * One shard of a table that spans 2^shard_bits GPUs (one process per GPU): the whole
 * table has 2^(l + shard_bits) slots, this map holds the slot range of shard_index.
 * The owner of a k-mer is the top shard_bits bits of its home slot.  Inserts and
 * lookups of k-mers that another shard owns are ignored / answer 0, so the same
 * batch can be offered to every shard.  shard_bits = 0 is tsx_hip_create.
 */
int tsx_hip_create_shard(tsx_hip_map **out, int k, int l, int storagebits, int overflow_l,
                         uint64_t hash_seed, int device, int shard_bits, int shard_index);
void tsx_hip_destroy(tsx_hip_map *m);
int tsx_hip_get_layout(const tsx_hip_map *m, tsx_hip_layout *out);
/* Zero the table, the secondary array and the counters (the counting mode stays). */
int tsx_hip_clear(tsx_hip_map *m);

/*
 * Canonical counting (jellyfish -C; no reference counterpart): a k-mer x and its reverse complement rc(x) share
 * one counter, so reads from both strands count as one sequence.  The key of the pair is min(h(x), h(rc x)) of
 * the hash mapping (the scan kernels roll the hash of the reverse complement alongside); a palindrome (x == rc(x),
 * even k) counts once per occurrence.  Every count and lookup entry point then works on pairs: a query for either
 * strand returns the pair's count, add_kmers adds to the pair, and the dumps report the LEXICOGRAPHICALLY smaller
 * strand (A < C < G < T, base 0 first).  The complement is taken on the 2-bit code (c -> 3 - c), so non-ACGT bytes
 * stay deterministic.  The multi-GPU merge (tsx_hip_group_merge) works on canonical tables; the sharded and
 * minimizer exchanges do not: tsx_hip_shard_*, tsx_hip_mini_* and tsx_hip_add_hashed_device refuse a canonical map
 * (TSX_HIP_EINVAL; the *_supported queries answer 0).
 *   set_canonical    on = 1 canonical, 0 forward (the default).  Only on an empty table -- just created or after
 *                    tsx_hip_clear -- and not on a map created with shard_bits > 0: TSX_HIP_EINVAL otherwise.
 *   canonical        the mode: 1 or 0.
 *   canonical_host   CPU only: out[i] = the lexicographically smaller of kmers[i] and its reverse complement, both
 *                    in the tsx_hip_encode layout (key_limbs(k) words per k-mer; out may equal kmers).
 */
int tsx_hip_set_canonical(tsx_hip_map *m, int on);
int tsx_hip_canonical(const tsx_hip_map *m);
int tsx_hip_canonical_host(int k, const uint64_t *kmers, size_t n, uint64_t *out);

/*
 * Base rule (jellyfish -Q and its non-ACGT rule; no reference counterpart): which windows of a sequence line are
 * k-mers.  Off by default: every window of k bytes counts, a non-ACGT byte as its stand-in code.
 *   acgt_only        1: a window is a k-mer only if all k of its bytes are in ACGTacgt.
 *   min_qual_char    c > 0: a window is a k-mer only if every base in it has a quality byte >= c (unsigned compare).
 *                    The quality of base j of a record's sequence line is byte j of the record's 4th non-empty line;
 *                    a base without one (a shorter quality line) counts as low quality.  FASTQ only: with 2-line
 *                    records the count and query entry points return TSX_HIP_EINVAL (tsx_hip_last_error says why).
 * The rule does not change keys: it may change between calls, and each call counts (or queries) under the rule in
 * effect then.  It holds for tsx_hip_count_fastq_host/_device/_bgzf_host (kmers_added counts only what it keeps) and
 * for tsx_hip_query_reads_* / tsx_hip_filter_reads_* (a dropped window is not a k-mer of the read).  Host pieces and
 * BGZF batches are cut at record boundaries under min_qual_char: a record longer than a piece (or than 8 MiB in a
 * BGZF file) gives TSX_HIP_ERANGE.  Like canonical tables, the sharded and minimizer exchanges refuse a table with a
 * rule (TSX_HIP_EINVAL; the *_supported queries answer 0); the group merge works.
 *   set_base_rule    acgt_only 0 or 1, min_qual_char 0 .. 255 (0 = off); a rule on a map created with
 *                    shard_bits > 0: TSX_HIP_EINVAL.
 *   get_base_rule    the rule in effect (either pointer may be NULL).
 */
int tsx_hip_set_base_rule(tsx_hip_map *m, int acgt_only, int min_qual_char);
int tsx_hip_get_base_rule(const tsx_hip_map *m, int *acgt_only, int *min_qual_char);
/* Wait for everything queued on the map's stream and report sticky errors
 * (TSX_HIP_EFULL / TSX_HIP_EOVERFLOW / TSX_HIP_ELOCK) raised by earlier inserts. */
int tsx_hip_sync(tsx_hip_map *m);

/*
 * countKMers (src/mains/main.cpp:104-218): FASTXreader<FASTQEntry>::getEntries
 * (FastXReader.h:221-280,307-385) + createKMers (testExecution.h:15-36) +
 * fromSequence + addKmer, for one whole FASTQ text.  Empty lines are skipped,
 * every 4 remaining lines are a record, line 2 is the sequence, every window
 * of k bytes of it is one k-mer.
 *
 * Both refuse a map created with shard_bits > 0 (TSX_HIP_EINVAL): a sharded table
 * is filled through tsx_hip_shard_scan_device / tsx_hip_shard_build_device.
 *
 * _host copies `n` bytes from host memory through pinned staging buffers.
 * _device takes a device pointer (16-byte aligned, text starts at a record
 * boundary), queues the work on `stream` (a hipStream_t, NULL = the map's own
 * stream) and returns without waiting; call tsx_hip_sync before reading.
 */
int tsx_hip_count_fastq_host(tsx_hip_map *m, const char *text, size_t n);
int tsx_hip_count_fastq_device(tsx_hip_map *m, const void *dev_text, size_t n, void *stream);

/*
 * Blocked gzip (BGZF, `bgzip`) input -- FastXReader.h:178-206 reads `.gz` through zlib (gzopen / gzgets), which
 * takes a BGZF file as ordinary multi-member gzip.  Here the members are found on the host (BC extra field) and
 * inflated ON THE DEVICE, one member per lane, CRC-32 and ISIZE of every member checked; the text never exists in
 * host memory.  tsx_hip_bgzf_index_host: TSX_HIP_EINVAL when the buffer is not BGZF (single-stream gzip: inflate it
 * with zlib and call tsx_hip_count_fastq_host).  tsx_hip_inflate_bgzf_host returns the inflated bytes (tests, tools).
 */
int tsx_hip_bgzf_index_host(const void *gz, size_t n, size_t *members, size_t *text_bytes);
int tsx_hip_inflate_bgzf_host(int device, const void *gz, size_t n, void *out_host, size_t out_cap, size_t *out_bytes);
int tsx_hip_count_fastq_bgzf_host(tsx_hip_map *m, const void *gz, size_t n);

/*
 * Lines per record of the texts handed to the count_fastq / shard_scan entry points: 4 = FASTQ
 * (FASTQEntry, FastXReader.h:62-95; the default), 2 = FASTA exactly as FASTXreader<FASTAEntry> reads it
 * (FastXReader.h:97-116: header line, ONE sequence line; sequences wrapped over several lines are not
 * joined there either).  Empty lines are dropped in both.  Wrapped FASTA has entry points of its own, which join the
 * lines and do not look at this setting: tsx_hip_count_fasta_host / _device / _bgzf_host below.
 */
int tsx_hip_set_record_lines(tsx_hip_map *m, int lines);

/*
 * Wrapped (multi-line) FASTA (csrc/tsx_fasta.h; no reference counterpart -- jellyfish and KMC join the lines too).  The
 * text is split at '\n' and empty lines are dropped; a line whose first byte is '>' is a header; the sequence of a record
 * is every other line up to the next header (or the end of the text), joined in order; lines in front of the first
 * header are a record of their own; a record without a sequence byte vanishes; a '>' elsewhere in a line and '\r' are
 * ordinary bytes.  Every window of k bytes of a record's sequence is a k-mer (stand-in codes, canonical mode and
 * acgt_only as everywhere): kmers_added grows by the sum of max(0, len - k + 1) over the records.  The lines are joined
 * on the device, piece by piece, into the text's two-line form -- ">\n" + sequence + "\n" per record, header text
 * dropped -- which the scan kernels then count; what a k-mer across two pieces needs travels in a device-resident carry.
 *   count_fasta_host       text in host memory, staged in pieces of TSX_HIP_PIECE_BYTES cut anywhere.
 *   count_fasta_device     a resident text (16-byte aligned) in windows of TSX_HIP_DEV_WINDOW (2 GiB at most); queued on
 *                          `stream` (NULL = the map's own), returns without waiting.
 *   count_fasta_bgzf_host  a BGZF image, batch after batch (TSX_HIP_BGZF_BATCH): inflated on the device, joined, counted.
 *                          TSX_HIP_EINVAL when the buffer is not BGZF.
 * All three count two-line records for the duration of the call whatever tsx_hip_set_record_lines says, and leave that
 * setting as they found it; a table built slab by slab keeps the whole two-line text resident, as
 * tsx_hip_count_fastq_host does.  TSX_HIP_EINVAL (tsx_hip_last_error says why): a map created with shard_bits > 0, a
 * base rule with min_qual_char (no quality line).
 *   unwrap_fasta_host      the two-line form of a whole text (one piece, whatever the window) into host memory: tests and
 *                          tools.  *out_bytes = its size, at most n + 2.  TSX_HIP_ERANGE for n >= 2^32 - 64 (*out_bytes
 *                          = n + 2 then) and when out_cap is too small (*out_bytes = the size needed).
 */
int tsx_hip_count_fasta_host(tsx_hip_map *m, const char *text, size_t n);
int tsx_hip_count_fasta_device(tsx_hip_map *m, const void *dev_text, size_t n, void *stream);
int tsx_hip_count_fasta_bgzf_host(tsx_hip_map *m, const void *gz, size_t n);
int tsx_hip_unwrap_fasta_host(int device, const char *text, size_t n, void *out_host, size_t out_cap, size_t *out_bytes);

/*
 * Measurement hooks (no reference counterpart): with timing enabled every
 * FASTQ piece records HIP events on its launch stream around the line passes,
 * around count_fastq_kernel and around the partition + segment-build kernels.
 * get_timing waits for them, returns the summed milliseconds of the three
 * phases and the number of pieces (= count_fastq_kernel launches), and resets
 * the accumulation.
 */
int tsx_hip_set_timing(tsx_hip_map *m, int enable);
int tsx_hip_get_timing(tsx_hip_map *m, double *line_ms, double *count_ms, double *build_ms,
                       uint64_t *launches);
/*
 * The same accumulation split per stage: stage_ms[7] = line passes, scan kernel
 * (count_fastq_kernel, or strip_desc_kernel + the walk), radix level 1 (offsets + partition; in a sharded run also the
 * histogram of the received keys), radix level 2, the segment build kernel, the gap between the end of the
 * scan and the start of the partition phase (0 except in a sharded run, where the owner split and the key
 * exchange lie there), and the inserts that wait for the build (overflow queues, deferred list).
 * Levels, build and inserts are 0 on the atomic path.  Either get_* call resets the accumulation.
 */
int tsx_hip_get_stage_timing(tsx_hip_map *m, double *stage_ms, uint64_t *launches);
/*
 * Insert path of the FASTQ entry points: 0 = choose per call (partitioned when
 * the text is at least 1/32 of the table bytes and k <= 32), 1 = always the
 * atomic path (one 64-bit CAS per distinct key), 2 = always the partitioned
 * path (keys radix-scattered by table segment, segments built in LDS).  Both
 * paths give identical tables up to slot order inside a segment.
 */
int tsx_hip_set_path(tsx_hip_map *m, int path);

/*
 * TSXHashMap::addKmer (TSXHashMap.h:182; CAS variant TSXHashMapCAS.h:268) for
 * a batch of n encoded k-mers; counts == NULL adds 1 per k-mer, otherwise
 * counts[i] occurrences (used by the multi-GPU merge).
 */
int tsx_hip_add_kmers_host(tsx_hip_map *m, const uint64_t *kmers, const uint64_t *counts, size_t n);
int tsx_hip_add_kmers_device(tsx_hip_map *m, const void *dev_kmers, const void *dev_counts, size_t n,
                             void *stream);

/* TSXHashMap::getKmerCount(kmer) (TSXHashMap.h:548-638) for n k-mers. */
int tsx_hip_get_counts_host(tsx_hip_map *m, const uint64_t *kmers, size_t n, uint64_t *counts_out);
int tsx_hip_get_counts_device(tsx_hip_map *m, const void *dev_kmers, size_t n, void *dev_counts_out,
                              void *stream);

/* getKmerCountDebug(kmer) (TSXHashMap.h:477-545): the count AND the slot the k-mer sits in
 * (KmerCountDebug::iFirstPos; UINT64_MAX when absent) -- main.cpp's --check marks these slots. */
int tsx_hip_lookup_host(tsx_hip_map *m, const uint64_t *kmers, size_t n, uint64_t *counts_out,
                        uint64_t *slots_out);
/* getKmerStarts / getKmerStartsRef (TSXHashMap.h:650-658) as a bitmap of 2^l bits: bit (i & 7) of
 * byte (i >> 3) is set iff slot i holds a k-mer.  nbytes >= 2^l / 8. */
int tsx_hip_kmer_starts_host(tsx_hip_map *m, uint8_t *bits_out, size_t nbytes);

/* getKmerCount() / print_stats() / iAddKmerCount (TSXHashMap.h:645,390; main.cpp:486-500). */
int tsx_hip_get_stats(tsx_hip_map *m, tsx_hip_stats *out);

/*
 * TSXHashMap::getAllKmers (TSXHashMap.h:660-722) plus each k-mer's count.
 * _device writes up to cap entries into device buffers (kmers: cap*key_limbs
 * uint64, counts: cap uint64) and the number written to *dev_n (uint64);
 * order is unspecified.  _host sizes with tsx_hip_get_stats().distinct.
 */
int tsx_hip_dump_host(tsx_hip_map *m, uint64_t *kmers_out, uint64_t *counts_out, size_t cap,
                      size_t *n_out);
int tsx_hip_dump_device(tsx_hip_map *m, void *dev_kmers_out, void *dev_counts_out, size_t cap,
                        void *dev_n, void *stream);
/*
 * Multi-GPU merge, sender side: like dump_device, but entries are grouped by
 * owner rank = tsx_hip_owner(kmer, nranks) into nranks contiguous segments;
 * dev_seg_counts (nranks uint64) receives the segment sizes.  The segments
 * travel through an RCCL all-to-all and are inserted on the owner with
 * tsx_hip_add_kmers_device.  cap must be >= distinct.
 */
int tsx_hip_partition_device(tsx_hip_map *m, int nranks, void *dev_kmers_out, void *dev_counts_out,
                             size_t cap, void *dev_seg_counts, void *stream);
/*
 * getAllKmers restricted to the table slots [slot_lo, slot_hi): a sample of the table for
 * cross-checks at sizes where the whole dump would not fit (bench.py's check).  cap must be
 * >= the number of occupied slots in the range (slot_hi - slot_lo always suffices).
 */
int tsx_hip_dump_range_device(tsx_hip_map *m, uint64_t slot_lo, uint64_t slot_hi, void *dev_kmers_out,
                              void *dev_counts_out, size_t cap, void *dev_n, void *stream);
int tsx_hip_owner_host(const tsx_hip_map *m, const uint64_t *kmer, int nranks);

/*
 * Counts out of the table, reduced on the device (csrc/tsx_output.h); both walk the slots like getAllKmers
 * (TSXHashMap.h:660-722) and leave the table as it is.
 *   histogram_device  abundance histogram of the slots [slot_lo, slot_hi) (jellyfish `histo`; no reference
 *                     counterpart): dev_hist (nbins uint64, zeroed by the call) gets hist[c] = k-mers counted exactly c
 *                     times for c < nbins - 1, hist[nbins - 1] = those counted nbins - 1 times or more; an occupied slot
 *                     whose count reads 0 lands in hist[0], so the sum is always the number of k-mers in the range.
 *                     nbins >= 2.  Queued on `stream` (NULL = the map's own), returns without waiting.
 *   histogram_host    the same over the whole table into host memory.
 */
int tsx_hip_histogram_device(tsx_hip_map *m, uint64_t slot_lo, uint64_t slot_hi, size_t nbins, void *dev_hist, void *stream);
int tsx_hip_histogram_host(tsx_hip_map *m, uint64_t *hist_out, size_t nbins);
/*
 * The `.count` file of count_kmers.py that main.cpp:224-396 reads back for --check: one line "kmer<TAB>count\n" per
 * k-mer whose count lies in [lower, upper] (bases as tsx_hip_decode writes them, the count in decimal; a canonical
 * table writes the lexicographically smaller strand, as the dumps do).  Order unspecified.
 *   format_counts_device  the text of the slots [slot_lo, slot_hi) into dev_text (cap bytes); *dev_nbytes and
 *                         *dev_nlines (uint64, device) receive its size.  Waits for the result; TSX_HIP_ERANGE when the
 *                         text does not fit (the buffer then holds part of it).  A line is at most k + 22 bytes.
 *   write_counts_host     the whole table to the file descriptor fd, chunk_bytes of device text at a time (0 = 256 MiB;
 *                         less than one line of k + 22 bytes: TSX_HIP_EINVAL); the device formats the next chunk while
 *                         the host writes one.  Lines and bytes written (optional).  A failed write: TSX_HIP_EIO.
 * Both: TSX_HIP_EINVAL for lower > upper.
 */
int tsx_hip_format_counts_device(tsx_hip_map *m, uint64_t slot_lo, uint64_t slot_hi, uint64_t lower, uint64_t upper,
                                 void *dev_text, size_t cap, void *dev_nbytes, void *dev_nlines, void *stream);
int tsx_hip_write_counts_host(tsx_hip_map *m, int fd, uint64_t lower, uint64_t upper, size_t chunk_bytes,
                              uint64_t *lines_out, uint64_t *bytes_out);

/*
 * K-mer database (csrc/tsx_db.h; no reference counterpart -- jellyfish `count -o` / `merge`): a lossless image of the
 * occupied slots of one table in a file, loaded back into a table or added to one.  Format version 1, little-endian
 * (DESIGN.md §3 "K-mer database"): a 128-byte header, one carry record per occupied entry of the secondary array
 * (pos, carry, the W words of slot pos), then chunks in slot order -- slot_lo, slot_hi, n_entries, checksum, one
 * occupancy bitmap word per 64 slots, the n_entries x W slot words as the table holds them -- and an end chunk with
 * slot_lo == slot_hi == 2^l, n_entries == 0.
 *   db_read_info  host only (no GPU): the header at offset 0 of fd (pread), magic, version and header checksum checked.
 *   save_host     the table to fd from its current position, chunk_bytes at most per chunk (0 = 256 MiB; too small for
 *                 64 slots: TSX_HIP_EINVAL); the device packs chunk i + 1 while the host writes chunk i.  Entries
 *                 (= distinct) and bytes written (optional).  A failed write: TSX_HIP_EIO.
 *   load_host     the database at the current position of fd into the table.  An empty table (just created or after
 *                 tsx_hip_clear) with the database's l, slot layout, segment bits and seed takes the slots as they are
 *                 (direct placement; the carries go through the secondary insert, so overflow_l may differ); any other
 *                 table gets every k-mer added with its count (re-insert: a different l or storage bits or seed, or a
 *                 table that already holds k-mers -- the load then merges by summing).  kmers_added grows by the
 *                 database's.  chunk_bytes: initial staging size (0 = 256 MiB; a larger chunk is staged whole); the
 *                 host reads chunk i + 1 while the device places chunk i.  Entries read (optional).
 * TSX_HIP_EFORMAT: bad magic or version, a checksum mismatch, a missing end marker (truncated file), chunks that do not
 * tile [0, 2^l), an occupied word with reprobe count 0 or LOCK set.  TSX_HIP_EINVAL: a different k, canonical mode or
 * base rule than the table's, a map created with shard_bits > 0.  After any error of load_host the table's content is
 * unspecified: tsx_hip_clear recovers it.  A tsx_hip_group is not saved or loaded (save each rank's map instead).
 */
typedef struct tsx_hip_db_info {
    uint32_t version;
    int32_t k, l;
    int32_t entry_limbs, func_bits, reprobe_bits, count_bits, seg_bits, overflow_l;   /* the slot layout (tsx_hip_layout) */
    int32_t canonical, acgt_only, min_qual_char;                                      /* counting mode and base rule */
    uint64_t hash_seed;
    uint64_t kmers_added, distinct, count_sum;                                        /* tsx_hip_stats at the save */
    uint64_t carry_records;
} tsx_hip_db_info;
int tsx_hip_db_read_info(int fd, tsx_hip_db_info *out);
int tsx_hip_save_host(tsx_hip_map *m, int fd, size_t chunk_bytes, uint64_t *entries_out, uint64_t *bytes_out);
int tsx_hip_load_host(tsx_hip_map *m, int fd, size_t chunk_bytes, uint64_t *entries_out);

/*
 * Read queries (csrc/tsx_query.h; no reference counterpart): run the records of a text against the table.  Records and
 * k-mers are exactly what counting the same text would count (FastXReader.h:62-116): empty lines are dropped, a record
 * is tsx_hip_set_record_lines consecutive non-empty lines (a trailing incomplete record is still one), its second line
 * is the sequence, every window of k bytes of it is one k-mer occurrence with the stand-in code of tsx_hip_encode for
 * non-ACGT bytes.  c(x) is getKmerCount(x) (TSXHashMap.h:548-638), 0 when x is absent; on a canonical table either
 * strand finds the pair's count.  Records are numbered from 0 in text order; per record:
 *   kmers      max(0, len - k + 1) of its sequence line
 *   in_range   windows with lower <= c <= upper, with multiplicity
 *   min_count  the smallest c, 0 when kmers = 0
 *   sum_count  the sum of c mod 2^64
 * Every query refuses a map created with shard_bits > 0 (a shard answers 0 for k-mers it does not own) and lower > upper
 * with TSX_HIP_EINVAL.
 *   query_reads_device  dev_text as tsx_hip_count_fastq_device takes it (16-byte aligned, starts at a record boundary);
 *                       queued on `stream` (NULL = the map's own) after what is queued there, the stats of records
 *                       [0, stats_cap) to dev_stats (zeroed by the call).  WAITS for the stream and reports the record
 *                       count to the host (*n_records, optional); more records than stats_cap: TSX_HIP_ERANGE (the first
 *                       stats_cap are written).
 *   query_reads_host    the same for text in host memory, taken in pieces cut at record boundaries, chunk_bytes at a
 *                       time (0 = 256 MiB; a record longer than a piece is taken whole); stats_out in host memory.
 */
typedef struct tsx_hip_read_stats {
    uint64_t kmers, in_range, min_count, sum_count;
} tsx_hip_read_stats;
int tsx_hip_query_reads_device(tsx_hip_map *m, const void *dev_text, size_t n, uint64_t lower, uint64_t upper,
                               void *dev_stats, size_t stats_cap, size_t *n_records, void *stream);
int tsx_hip_query_reads_host(tsx_hip_map *m, const char *text, size_t n, uint64_t lower, uint64_t upper,
                             tsx_hip_read_stats *stats_out, size_t stats_cap, size_t *n_records, size_t chunk_bytes);
/*
 * Read filter: a record passes iff in_range >= min_in_range and in_range * 10^6 >= fraction_ppm * kmers (so a record
 * shorter than k passes when min_in_range = 0); invert != 0 writes the records that fail instead.  A written record is
 * its bytes from the first byte of its first line through the '\n' that ends its last line ('\n' added when the text
 * ends without one); empty lines between records are not written; output is in input order.  TSX_HIP_EINVAL also for
 * fraction_ppm > 10^6.
 *   filter_reads_host    text in host memory, in pieces as query_reads_host; the device compacts each piece while the
 *                        host writes the previous one to fd.  Records kept and bytes written (optional).  A failed write:
 *                        TSX_HIP_EIO.
 *   filter_reads_device  the whole of dev_text (as query_reads_device; n < 3.75 GiB) into dev_out (16-byte aligned,
 *                        out_cap >= n + 64, else TSX_HIP_ERANGE); *out_bytes = the output's size.  Waits for the stream.
 */
typedef struct tsx_hip_filter_rule {
    uint64_t lower, upper;      /* the count range of an in_range window */
    uint64_t min_in_range;      /* windows in range a record needs */
    uint32_t fraction_ppm;      /* share of its windows that must be in range, in millionths (10^6 = all) */
    int32_t invert;             /* write the records that fail */
} tsx_hip_filter_rule;
int tsx_hip_filter_reads_host(tsx_hip_map *m, const char *text, size_t n, const tsx_hip_filter_rule *rule, int fd,
                              size_t chunk_bytes, uint64_t *kept_out, uint64_t *bytes_out);
int tsx_hip_filter_reads_device(tsx_hip_map *m, const void *dev_text, size_t n, const tsx_hip_filter_rule *rule,
                                void *dev_out, size_t out_cap, size_t *out_bytes, uint64_t *kept_out, void *stream);
/*
 * Sequence queries (csrc/tsx_seq.h; no reference counterpart -- Merqury's QV and asm_only.bed, KAT sect): the sequences
 * of a WRAPPED (multi-line) FASTA text against the table.  The records are those of tsx_hip_count_fasta_*: lines in front
 * of the first header form a record with the empty name, a record without a sequence byte vanishes, sequences are
 * numbered from 0 in text order counting only the records that remain.  A sequence's name is its header behind the '>'
 * up to the first space or tab, cut to TSX_HIP_SEQ_NAME_MAX bytes.  Windows, k-mers (under the table's base rule) and c(x)
 * are those of tsx_hip_query_reads_* on the joined sequence.  Per sequence (tsx_hip_seq_stats):
 *   length     its sequence bytes
 *   kmers      windows that are k-mers under the base rule
 *   present    those with lower <= c <= upper
 *   min_count  the smallest c, 0 when kmers = 0;  sum_count  the sum of c mod 2^64
 * A MISSING window is a k-mer with c outside lower..upper; tsx_hip_seq_interval {seq, start, end} is a maximal run of
 * consecutive missing start positions s..e as the half-open base interval [s, e + k) of the joined sequence (a window
 * the base rule drops ends a run), ordered by sequence, then start.
 * The calls take the text in pieces cut ANYWHERE (chunk_bytes at a time, 0 = 256 MiB, at most TSX_HIP_PIECE_BYTES when
 * that is set; TSX_HIP_DEV_WINDOW for a device text; TSX_HIP_BGZF_BATCH for a BGZF image): what identifies a sequence
 * across a seam travels in a carry.  Results come in a tsx_hip_seq_result the caller frees; *res is NULL on failure.
 * The _missing_ calls fill the stats and the intervals, the _stats_ calls the stats only.  Refused with TSX_HIP_EINVAL
 * (tsx_hip_last_error says which): lower > upper, a map created with shard_bits > 0, min_qual_char set on the table (a
 * FASTA text has no quality line).
 *   tsx_hip_seq_write_stats    one line per sequence to fd: name, length, kmers, present, missing (kmers - present), min,
 *                              sum, qv, tab-separated; qv = -10 log10(1 - (present / kmers)^(1 / k)) as %.4f, "inf" when
 *                              nothing is missing, "NA" without k-mers; an empty name is written "*".
 *   tsx_hip_seq_write_missing  BED: name, start, end.
 */
#define TSX_HIP_SEQ_NAME_MAX 255
typedef struct tsx_hip_seq_stats {
    uint64_t length, kmers, present, min_count, sum_count;
} tsx_hip_seq_stats;
typedef struct tsx_hip_seq_interval {
    uint64_t seq, start, end;
} tsx_hip_seq_interval;
typedef struct tsx_hip_seq_result tsx_hip_seq_result;
int tsx_hip_seq_stats_host(tsx_hip_map *m, const char *text, size_t n, uint64_t lower, uint64_t upper, size_t chunk_bytes,
                           tsx_hip_seq_result **res);
int tsx_hip_seq_stats_bgzf_host(tsx_hip_map *m, const void *gz, size_t n, uint64_t lower, uint64_t upper,
                                tsx_hip_seq_result **res);
int tsx_hip_seq_stats_device(tsx_hip_map *m, const void *dev_text, size_t n, uint64_t lower, uint64_t upper,
                             tsx_hip_seq_result **res, void *stream);
int tsx_hip_seq_missing_host(tsx_hip_map *m, const char *text, size_t n, uint64_t lower, uint64_t upper, size_t chunk_bytes,
                             tsx_hip_seq_result **res);
int tsx_hip_seq_missing_bgzf_host(tsx_hip_map *m, const void *gz, size_t n, uint64_t lower, uint64_t upper,
                                  tsx_hip_seq_result **res);
int tsx_hip_seq_missing_device(tsx_hip_map *m, const void *dev_text, size_t n, uint64_t lower, uint64_t upper,
                               tsx_hip_seq_result **res, void *stream);
size_t tsx_hip_seq_result_count(const tsx_hip_seq_result *res);
const tsx_hip_seq_stats *tsx_hip_seq_result_stats(const tsx_hip_seq_result *res);
/* the names back to back; name i is bytes [offsets[i], offsets[i + 1]) (count + 1 offsets) */
const char *tsx_hip_seq_result_names(const tsx_hip_seq_result *res, const uint64_t **offsets);
size_t tsx_hip_seq_result_intervals(const tsx_hip_seq_result *res, const tsx_hip_seq_interval **intervals);
void tsx_hip_seq_result_free(tsx_hip_seq_result *res);
int tsx_hip_seq_write_stats(const tsx_hip_seq_result *res, int k, int fd);
int tsx_hip_seq_write_missing(const tsx_hip_seq_result *res, int fd);
/*
 * Coverage tracks (csrc/tsx_track.h; no reference counterpart -- KAT sect, the copy-number track next to Merqury's
 * spectra-cn): the k-mer counts of every sequence in bins along it.  Sequences, names, length, k-mers, c(x), lower..upper
 * and "present" are those of tsx_hip_seq_stats_*.  A sequence of length L has ceil(L / window) bins (none for L = 0); bin
 * b covers the START positions [b * window, min((b + 1) * window, L)) of the joined sequence.  Per bin (tsx_hip_seq_bin):
 *   kmers      start positions of the bin whose window is a k-mer (the last k - 1 of a sequence never are)
 *   present    those with lower <= c <= upper
 *   min_count, max_count  the smallest and the largest c, both 0 when kmers = 0;  sum_count  the sum of c mod 2^64
 * A sequence's bins sum to its tsx_hip_seq_stats row.  The track calls fill the stats and the names as the _stats_ calls
 * do, and no intervals; the result does not depend on where the pieces of the text are cut.  Refused with
 * TSX_HIP_EINVAL (tsx_hip_last_error says which): what the _stats_ calls refuse, and a window outside 64 .. 2^32.
 *   tsx_hip_seq_result_bins    the bins of all sequences back to back; those of sequence i are [first[i], first[i + 1])
 *                              (count + 1 offsets).  Returns their number; a result without a track: 0 and NULL.
 *   tsx_hip_seq_result_window  the window of the result's track, 0 for a result without one.
 *   tsx_hip_seq_write_track    one line per bin to fd: name, start, end, kmers, present, min, max, mean, tab-separated;
 *                              mean = sum / kmers as %.4f, "NA" when kmers = 0; an empty name is written "*".  A result
 *                              without a track: TSX_HIP_EINVAL; a failed write: TSX_HIP_EIO.
 */
typedef struct tsx_hip_seq_bin {
    uint64_t kmers, present, min_count, max_count, sum_count;
} tsx_hip_seq_bin;
int tsx_hip_seq_track_host(tsx_hip_map *m, const char *text, size_t n, uint64_t lower, uint64_t upper, uint64_t window,
                           size_t chunk_bytes, tsx_hip_seq_result **res);
int tsx_hip_seq_track_bgzf_host(tsx_hip_map *m, const void *gz, size_t n, uint64_t lower, uint64_t upper, uint64_t window,
                                tsx_hip_seq_result **res);
int tsx_hip_seq_track_device(tsx_hip_map *m, const void *dev_text, size_t n, uint64_t lower, uint64_t upper, uint64_t window,
                             tsx_hip_seq_result **res, void *stream);
size_t tsx_hip_seq_result_bins(const tsx_hip_seq_result *res, const tsx_hip_seq_bin **bins, const uint64_t **first);
uint64_t tsx_hip_seq_result_window(const tsx_hip_seq_result *res);
int tsx_hip_seq_write_track(const tsx_hip_seq_result *res, int fd);
/*
 * Read trimming (csrc/tsx_trim.h; no reference counterpart -- khmer `filter-abund` / `trim-low-abund`, Quake, Lighter):
 * keep of every record the stretch of its sequence whose k-mers are trusted.  Records, lines, k-mers and c(x) are those
 * of tsx_hip_query_reads_*, and the table's base rule (tsx_hip_set_base_rule) decides which windows are k-mers at all.
 * Window i of a sequence line of length L (0 <= i <= L - k) is SOLID when it is a k-mer under the base rule and
 * lower <= c(x) <= upper.  A RUN is a maximal stretch of consecutive solid windows [i, j]; it covers bases [i, j + k).
 * `mode` picks the run that decides the record's kept span:
 *   TSX_HIP_TRIM_LONGEST  the longest run, the leftmost among equals
 *   TSX_HIP_TRIM_PREFIX   the run that contains window 0 (none when window 0 is not solid): cut at the first untrusted k-mer
 * The span is (start, length) in bases of the sequence line, (0, 0) without a run; a non-empty span is >= k long (and,
 * like a sequence line, shorter than 4 GiB).
 * A record is WRITTEN when length >= min_len (0 = k; a record of length 0 is never written).  A written record is, in
 * order: its first line, whole; bytes [start, start + length) of the sequence line; for 4-line records the third line,
 * whole, and bytes [min(start, Lq), min(start + length, Lq)) of the quality line of length Lq -- each followed by '\n'
 * (also where the text's last line lacks one).  A trailing incomplete record writes the lines it has, by the same
 * rules.  Output is in input order; empty lines of the input are not written.
 * TSX_HIP_EINVAL for a map created with shard_bits > 0, lower > upper, an unknown mode and reserved != 0.
 *   trim_spans_device  dev_text as tsx_hip_query_reads_device takes it; the spans of records [0, spans_cap) to dev_spans
 *                      (tsx_hip_trim_span each, zeroed by the call; min_len plays no part).  WAITS for the stream; more
 *                      records than spans_cap: TSX_HIP_ERANGE (the first spans_cap are written).
 *   trim_spans_host    the same for text in host memory, in pieces as tsx_hip_query_reads_host (chunk_bytes 0 = 256 MiB).
 *   trim_reads_device  the written records of the whole of dev_text (n < 3.75 GiB) into dev_out (16-byte aligned,
 *                      out_cap >= n + 64, else TSX_HIP_ERANGE); totals->bytes = the output's size.  Waits for the stream.
 *   trim_reads_host    text in host memory in pieces; the device trims piece i + 1 while the host writes piece i to fd.
 *                      A failed write: TSX_HIP_EIO.
 * totals (optional): records seen, records written, bases of all sequence lines, bases written, bytes written.
 */
#define TSX_HIP_TRIM_LONGEST 0
#define TSX_HIP_TRIM_PREFIX 1
typedef struct tsx_hip_trim_rule {
    uint64_t lower, upper;      /* the count range of a solid window */
    uint64_t min_len;           /* bases a record must keep to be written (0 = k) */
    int32_t mode;               /* TSX_HIP_TRIM_* */
    int32_t reserved;           /* 0 */
} tsx_hip_trim_rule;
typedef struct tsx_hip_trim_span {
    uint64_t start, length;
} tsx_hip_trim_span;
typedef struct tsx_hip_trim_totals {
    uint64_t records, kept, bases_in, bases_kept, bytes;
} tsx_hip_trim_totals;
int tsx_hip_trim_spans_device(tsx_hip_map *m, const void *dev_text, size_t n, const tsx_hip_trim_rule *rule,
                              void *dev_spans, size_t spans_cap, size_t *n_records, void *stream);
int tsx_hip_trim_spans_host(tsx_hip_map *m, const char *text, size_t n, const tsx_hip_trim_rule *rule,
                            tsx_hip_trim_span *spans_out, size_t spans_cap, size_t *n_records, size_t chunk_bytes);
int tsx_hip_trim_reads_device(tsx_hip_map *m, const void *dev_text, size_t n, const tsx_hip_trim_rule *rule,
                              void *dev_out, size_t out_cap, tsx_hip_trim_totals *totals, void *stream);
int tsx_hip_trim_reads_host(tsx_hip_map *m, const char *text, size_t n, const tsx_hip_trim_rule *rule, int fd,
                            size_t chunk_bytes, tsx_hip_trim_totals *totals);

/*
 * Read correction (csrc/tsx_correct.h; no reference counterpart -- Quake, Musket, Lighter, BFC): undo single
 * substitutions that the k-mer spectrum identifies exactly.  Records, lines and SOLID windows are those of
 * tsx_hip_trim_* (a k-mer under the table's base rule whose count lies in lower..upper).  A sequence line of length L
 * has n = L - k + 1 windows.  Of the maximal runs [a, b] of non-solid windows, w = b - a + 1, a run is a SITE with
 * suspect base p when
 *   interior  a > 0, b < n - 1 and w == k:   p = b
 *   head      a == 0, b < n - 1 and w <= k:  p = b
 *   tail      a > 0, b == n - 1 and w <= k:  p = a + k - 1
 * and w >= min_windows; no other run is one (the whole read, an interior run shorter or longer than k, n < 2).  The
 * windows that hold p are exactly a..b, so sites never share a window and each is judged on the original text: no passes,
 * no order.  A site whose byte at p is not in ACGTacgt is UNFIXABLE.  Alternative d = 1..3 replaces the code c of that
 * byte by c ^ d and is GOOD when every window a..b is solid with the replacement.  Exactly one good alternative: the site
 * is CORRECTED, the byte becomes "ACGT"[c ^ d] in the case of the original; two or three: AMBIGUOUS; none: UNFIXABLE;
 * both untouched.  Every other byte of the text stays as it is; one call is one round.
 * TSX_HIP_EINVAL (tsx_hip_last_error says which) for a map created with shard_bits > 0, a table with min_qual_char set
 * (its dropped windows would make every low-quality base a site for ever), lower > upper, min_windows outside 1..k,
 * reserved != 0, a NULL rule.
 *   correct_sites_device  dev_text as tsx_hip_trim_spans_device takes it; the corrections [0, cap) to dev_corrections
 *                         (tsx_hip_correction each, in no order).  WAITS for the stream; more corrections than cap:
 *                         TSX_HIP_ERANGE (cap of them are written, *n_corrections says how many there are).
 *   correct_sites_host    text in host memory in pieces cut at record boundaries (chunk_bytes 0 = 256 MiB, at most
 *                         TSX_HIP_PIECE_BYTES); the corrections sorted by (record, pos); more than cap: TSX_HIP_ERANGE
 *                         with the first cap of that order written.
 *   correct_reads_device  the n bytes of dev_text with the corrections applied into dev_out (out_cap >= n, else
 *                         TSX_HIP_ERANGE; dev_out may be dev_text).  Waits for the stream.
 *   correct_reads_host    the same to fd, piece by piece behind the device; exactly n bytes.  A failed write: TSX_HIP_EIO.
 * totals (optional): records seen, sites = corrected + ambiguous + unfixable, bytes written (0 for the sites calls).
 */
typedef struct tsx_hip_correct_rule {
    uint64_t lower, upper;      /* the count range of a solid window */
    uint32_t min_windows;       /* a run of fewer non-solid windows is no site (1..k) */
    uint32_t reserved;          /* 0 */
} tsx_hip_correct_rule;
typedef struct tsx_hip_correction {
    uint64_t record;            /* the record's index in the text */
    uint32_t pos;               /* the base's offset in its sequence line */
    uint8_t from, to;           /* the byte that was there, the byte that replaces it */
    uint16_t windows;           /* w: the non-solid windows the correction makes solid */
} tsx_hip_correction;
typedef struct tsx_hip_correct_totals {
    uint64_t records, sites, corrected, ambiguous, unfixable, bytes;
} tsx_hip_correct_totals;
int tsx_hip_correct_sites_device(tsx_hip_map *m, const void *dev_text, size_t n, const tsx_hip_correct_rule *rule,
                                 void *dev_corrections, size_t cap, size_t *n_corrections, tsx_hip_correct_totals *totals,
                                 void *stream);
int tsx_hip_correct_sites_host(tsx_hip_map *m, const char *text, size_t n, const tsx_hip_correct_rule *rule,
                               tsx_hip_correction *corrections_out, size_t cap, size_t *n_corrections,
                               tsx_hip_correct_totals *totals, size_t chunk_bytes);
int tsx_hip_correct_reads_device(tsx_hip_map *m, const void *dev_text, size_t n, const tsx_hip_correct_rule *rule,
                                 void *dev_out, size_t out_cap, tsx_hip_correct_totals *totals, void *stream);
int tsx_hip_correct_reads_host(tsx_hip_map *m, const char *text, size_t n, const tsx_hip_correct_rule *rule, int fd,
                               size_t chunk_bytes, tsx_hip_correct_totals *totals);

/*
 * Read medians (csrc/tsx_median.h; no reference counterpart -- khmer `count-median` / `normalize-by-median`, KAT `sect`,
 * `jellyfish query -s`): the count of every window of a text, and per record the median of them.  Records, lines,
 * k-mers and c(x) are those of tsx_hip_query_reads_*; the table's base rule (tsx_hip_set_base_rule) decides which
 * windows are k-mers, exactly as for tsx_hip_trim_*.  On a canonical table either strand finds the pair's count.
 * PROFILE: one uint32_t per byte of the text.  Entry i is min(c(x), 0xFFFFFFFE) when a window that is a k-mer (on a
 *   sequence line, under the base rule) starts at byte i, and TSX_HIP_NO_KMER otherwise: header, '+' and quality lines,
 *   the last k - 1 bytes of a sequence line and its '\n', empty lines, windows the base rule drops.
 * MEDIAN of a record: with v_0 <= ... <= v_(m-1) the profile entries of its k-mers, sorted (the saturated values; m =
 *   `kmers`), the median is v_(m/2) (integer division: the upper middle for even m, khmer's convention), and 0 when
 *   m = 0.  `kmers` counts k-mers under the base rule: it equals tsx_hip_read_stats.kmers when no base rule is set.
 * MEDIAN RULE: a record passes iff lower <= median <= upper (a record with m = 0 is judged by its median 0); invert != 0
 *   writes the records that fail.  What a written record is, the order and the '\n' handling are those of
 *   tsx_hip_filter_reads_host.
 * TSX_HIP_EINVAL for a map created with shard_bits > 0, and for a rule that is NULL, has lower > upper or reserved != 0.
 *   count_profile_device  dev_text as tsx_hip_query_reads_device takes it; dev_profile: n uint32_t in device memory,
 *                         every one written once.  WAITS for the stream.
 *   count_profile_host    the same for text in host memory, in pieces cut at record boundaries (chunk_bytes 0 = 256 MiB,
 *                         and at most TSX_HIP_PIECE_BYTES when that is set; a record longer than a piece is taken
 *                         whole); profile positions are text positions.
 *   median_reads_device   {kmers, median} of records [0, cap) to dev_medians (tsx_hip_read_median each).  The profile
 *                         of the whole text (4 n bytes) and the line offsets are scratch of the call.  WAITS for the
 *                         stream; more records than cap: TSX_HIP_ERANGE (the first cap are written).
 *   median_reads_host     the same for text in host memory, in pieces.
 *   filter_median_host    text in host memory in pieces; the device compacts piece i + 1 while the host writes piece i to
 *                         fd.  Records kept and bytes written (optional).  A failed write: TSX_HIP_EIO.
 * A record whose sequence line is longer than TSX_HIP_MEDIAN_LONG bases (environment, read per call; default 16384, at
 * least 64) is selected by a whole workgroup instead of one wave; the results do not depend on it.
 */
#define TSX_HIP_NO_KMER 0xFFFFFFFFu
typedef struct tsx_hip_read_median {
    uint64_t kmers, median;
} tsx_hip_read_median;
typedef struct tsx_hip_median_rule {
    uint64_t lower, upper;      /* the range of a passing median */
    int32_t invert;             /* write the records that fail */
    int32_t reserved;           /* 0 */
} tsx_hip_median_rule;
int tsx_hip_count_profile_device(tsx_hip_map *m, const void *dev_text, size_t n, void *dev_profile, void *stream);
int tsx_hip_count_profile_host(tsx_hip_map *m, const char *text, size_t n, uint32_t *profile_out, size_t chunk_bytes);
int tsx_hip_median_reads_device(tsx_hip_map *m, const void *dev_text, size_t n, void *dev_medians, size_t cap,
                                size_t *n_records, void *stream);
int tsx_hip_median_reads_host(tsx_hip_map *m, const char *text, size_t n, tsx_hip_read_median *out, size_t cap,
                              size_t *n_records, size_t chunk_bytes);
int tsx_hip_filter_median_host(tsx_hip_map *m, const char *text, size_t n, const tsx_hip_median_rule *rule, int fd,
                               size_t chunk_bytes, uint64_t *kept_out, uint64_t *bytes_out);

/*
 * Digital normalization (csrc/tsx_normalize.h; no reference counterpart -- khmer `normalize-by-median`): the records of
 * a text are kept while the median count of their k-mers, among the records kept so far, is below a cutoff, and only
 * the k-mers of kept records are counted.  Records, lines, k-mers, the base rule and canonical keys are those of
 * tsx_hip_median_reads_*; records are numbered from 0 over the whole text.
 * ROUNDS: with R = round_records >= 1, round j holds the records [j R, (j + 1) R); the last round may be short.  For
 *   each round in order: every record of the round gets its median (the MEDIAN above: saturated counts, v_(m/2), 0 for a
 *   record without k-mers) against the table as it stands; a record is KEPT iff median < cutoff; after the whole round is
 *   judged, every k-mer occurrence of its kept records is added to the table.  R = 1 is khmer's sequential rule.
 *   The result depends on R and on nothing else: not on chunk_bytes, TSX_HIP_PIECE_BYTES, TSX_HIP_DEV_WINDOW or
 *   TSX_HIP_MEDIAN_LONG.  TSX_HIP_NORMALIZE_ROUND (65536) is the R of the tools; it is part of the result's definition.
 *   cutoff = 0 keeps nothing and leaves the table as it was; cutoff = UINT64_MAX keeps everything and leaves the table
 *   of tsx_hip_count_fastq_host.  The table need not be empty at the start.
 * OUTPUT: kept records are written whole, in input order, exactly as tsx_hip_filter_reads_host writes a record.
 * TOTALS: records and kept records, the k-mers of all records (kmers_seen) and of the kept ones (kmers_added), rounds.
 * The k-mers go in by the atomic insert path into a whole table: TSX_HIP_EINVAL (with a tsx_hip_last_error text) for a
 *   map created with shard_bits > 0, a table above 2^32 slots (built slab by slab), an armed prefilter, a NULL rule,
 *   round_records == 0 or reserved != 0.  A full table is reported as by the counting calls (tsx_hip_sync).
 *   normalize_host    text in host memory, in pieces cut at ROUND boundaries (chunk_bytes 0 = 256 MiB, at most
 *                     TSX_HIP_PIECE_BYTES when that is set; a round longer than a piece is taken whole).  fd >= 0: the
 *                     kept records go to fd, piece i written while the device works on piece i + 1 (a failed write:
 *                     TSX_HIP_EIO); fd = -1: no output.  keep_out (NULL, or keep_cap bytes): 1 for a kept record, else
 *                     0.  More records than keep_cap: TSX_HIP_ERANGE; the first keep_cap entries are written and the
 *                     table is complete.
 *   normalize_device  dev_text as tsx_hip_median_reads_device takes it; dev_keep: keep_cap bytes in device memory, as
 *                     keep_out.  The profile of the whole text and the line offsets are scratch of the call.  WAITS for
 *                     the stream.
 */
#define TSX_HIP_NORMALIZE_ROUND 65536u
typedef struct tsx_hip_normalize_rule {
    uint64_t cutoff;            /* keep a record iff its median < cutoff */
    uint64_t round_records;     /* R >= 1 */
    int32_t reserved[2];        /* 0 */
} tsx_hip_normalize_rule;
typedef struct tsx_hip_normalize_totals {
    uint64_t records, kept, kmers_seen, kmers_added, rounds;
} tsx_hip_normalize_totals;
int tsx_hip_normalize_host(tsx_hip_map *m, const char *text, size_t n, const tsx_hip_normalize_rule *rule, int fd,
                           uint8_t *keep_out, size_t keep_cap, size_t chunk_bytes, tsx_hip_normalize_totals *totals);
int tsx_hip_normalize_device(tsx_hip_map *m, const void *dev_text, size_t n, const tsx_hip_normalize_rule *rule,
                             void *dev_keep, size_t keep_cap, tsx_hip_normalize_totals *totals, void *stream);

/*
 * Table sizing (csrc/tsx_sketch.h; no reference counterpart -- ntCard / KmerStream in front of KMC, jellyfish grows its
 * table): a HyperLogLog sketch of the k-mers a text WOULD put into a table, its estimate of their distinct number, and
 * the l that holds them.  Nothing is counted and no table is read or written.
 * ELEMENTS: every window the counting calls would count (records, lines and the base rule of tsx_hip_set_base_rule as
 *   for tsx_hip_query_reads_*; non-ACGT bytes stand for the codes tsx_hip_encode gives them) is one element: the k-mer
 *   x in the tsx_hip_encode layout, WK = tsx_hip_key_limbs(k) limbs; on a canonical map the lexicographically smaller of
 *   x and rc(x) (tsx_hip_canonical_host).  NOT the table's hashed key: a sketch depends on neither l, storagebits nor
 *   the seed, and sketches of several texts and maps combine by the register-wise maximum.  The distinct elements are
 *   the slots the table would occupy (its key is a bijection of exactly this element).
 * HASH: v = 0x9E3779B97F4A7C15; for t = 0 .. WK-1: v = mix64(v ^ x[t]), with the splitmix64 finaliser
 *   mix64(z): z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; return z ^ z >> 31.
 * REGISTERS: 2^p of them, precision p = 10 .. 14; idx = v >> (64 - p), rank = 1 + clz((v << p) | 1 << (p - 1)) (1 ..
 *   64 - p + 1), M[idx] = max(M[idx], rank).  One uint8_t per register on the host, one uint32_t on the device.
 * ESTIMATE: m = 2^p, E = a m^2 / sum_j 2^-M[j] with a = 0.7213 / (1 + 1.079 / m); when E <= 2.5 m and V > 0 registers
 *   are zero, E = m ln(m / V) (linear counting).  No large-range correction (a 64-bit hash).  The sum runs over a rank
 *   histogram, ranks ascending.  Standard error 1.04 / sqrt(m): 0.81 % at p = 14.
 * TSX_HIP_EINVAL, before any GPU call: precision outside 10 .. 14, a NULL map or regs, text NULL with n > 0, a device
 * text that is not 16-byte aligned.  The map supplies k, the record lines, canonical and the base rule; it may be empty
 * or filled, whole or a shard (shard_bits > 0).  Wrapped FASTA has no sketch (tsx_hip_set_record_lines takes 2 or 4).
 *   sketch_host        text in host memory, in pieces cut at record boundaries (chunk_bytes 0 = 256 MiB, and at most
 *                      TSX_HIP_PIECE_BYTES when that is set).  regs[2^p] is IN/OUT: the registers of the text are
 *                      max-combined into it, so several texts accumulate into one sketch.  *totals (optional) is added
 *                      to: kmers = the exact number of elements, records = the records read.
 *   sketch_bgzf_host   the same for the image of a BGZF file, inflated on the device in batches (TSX_HIP_BGZF_BATCH).
 *   sketch_device      dev_text as tsx_hip_query_reads_device takes it (windows of TSX_HIP_DEV_WINDOW); dev_regs:
 *                      uint32_t[2^p] in device memory, in/out; dev_totals: two uint64_t {kmers, records} in device
 *                      memory, added to, or NULL.  Queued on the stream, not waited for.
 *   sketch_kmers_host  CPU only: the n elements kmers[i * WK ..] as given (the caller canonicalises), into regs.
 *   sketch_estimate_host  CPU only: E of regs[2^p]; 0 for an all-zero sketch; < 0 for bad arguments (a register above
 *                      64 - p + 1 among them).
 *   suggest_l          CPU only: need = distinct * (1 + 5 * 1.04 / sqrt(2^p)) / (load_ppm / 1e6) -- five standard
 *                      errors of margin at the load asked for -- and *l_out = the smallest l with 2^l >= need, at least
 *                      4 and at most min(36, 2k - 1).  load_ppm 0 = 750000; above 900000: TSX_HIP_EINVAL.  When the
 *                      upper bound leaves distinct / 2^l above 0.9: TSX_HIP_ERANGE, *l_out set to that bound.  (A long
 *                      k-mer has no layout at a small l -- tsx_hip_create refuses k = 127 below l = 11: callers take the
 *                      smallest l that creates, as tsxCount --l=auto and TSXHashMapHIP.sizedFor do.)
 */
typedef struct tsx_hip_sketch_totals {
    uint64_t kmers, records;
} tsx_hip_sketch_totals;
int tsx_hip_sketch_host(tsx_hip_map *m, const char *text, size_t n, int precision, uint8_t *regs,
                        tsx_hip_sketch_totals *totals, size_t chunk_bytes);
int tsx_hip_sketch_bgzf_host(tsx_hip_map *m, const void *gz, size_t n, int precision, uint8_t *regs,
                             tsx_hip_sketch_totals *totals);
int tsx_hip_sketch_device(tsx_hip_map *m, const void *dev_text, size_t n, int precision, void *dev_regs, void *dev_totals,
                          void *stream);
int tsx_hip_sketch_kmers_host(int k, const uint64_t *kmers, size_t n, int precision, uint8_t *regs);
double tsx_hip_sketch_estimate_host(const uint8_t *regs, int precision);
int tsx_hip_suggest_l(int k, double distinct, int precision, uint32_t load_ppm, int *l_out);

/*
 * Counting only the k-mers seen twice (csrc/tsx_prefilter.h; no reference counterpart -- jellyfish --bf-size, BFCounter,
 * KMC -ci2): a prefilter that belongs to a map, filled in a first pass over the input; the counting calls consult it in a
 * second pass over the same input, so that a k-mer that occurs once takes no slot of the table.
 * ELEMENT and HASH: exactly the sketch's (above): the k-mer x in the tsx_hip_encode layout, WK limbs, on a canonical map
 *   the lexicographically smaller strand; windows, records and the base rule are those of the counting calls;
 *   v = sketch hash of x.  The filters depend on neither l, storagebits nor the seed.
 * FILTERS: two blocked Bloom filters of 64-bit words.  A ("seen") has 2^bits bits, B ("seen again") 2^(bits - 2);
 *   12 <= bits <= 38.  WORD of a key: v >> (64 - (bits - 6)) in A, v >> (64 - (bits - 8)) in B.  MASK, the same in both:
 *   the OR of 1 << ((v >> s) & 63) for s = 0, 6, 12, 18 (one to four bits).  In a filter: (word & mask) == mask.
 * PASS 1 (prefilter_add_*): every window ORs its mask into A (one returning 64-bit atomic); when A already held the
 *   mask -- or the window's equal neighbour just did the same -- it ORs the mask into B.  Several calls accumulate.
 * PASS 2 (while armed): tsx_hip_count_fastq_host / _device / _bgzf_host insert the windows whose mask is in B and skip
 *   the others.  They take the atomic insert path whatever tsx_hip_set_path says.  Not gated: tsx_hip_add_kmers_*,
 *   tsx_hip_load_host, tsx_hip_combine, every read call.  tsx_hip_get_stats' kmers counts the inserted windows only.
 * CONTRACT: after pass 1 and pass 2 over the same input, EVERY k-mer that occurs at least twice is in the table with its
 *   exact count.  A k-mer that occurs once is absent, or -- a false positive of B -- present with count 1.  So a dump
 *   with lower >= 2, histogram bins >= 2 and every read call with a lower bound >= 2 are those of an unfiltered count;
 *   the false-positive rate decides the slots saved, never a count.
 * STREAMS: B must be complete before pass 2 reads it, and the library sees to that itself.  prefilter_create returns
 *   with the filters zeroed (it waits).  An armed counting call first orders its stream behind the map's own stream and
 *   behind the stream of the last *_device call on this map, so pass 1 through any prefilter_add_* followed by pass 2
 *   through any counting call needs nothing from the caller.  Only a caller that runs pass 1 on SEVERAL streams of its
 *   own at once joins them (or calls tsx_hip_sync, which waits for the last one) before the armed count.
 * tsx_hip_clear empties the table and leaves the prefilter alone: the filters, armed or not, and the totals of
 *   prefilter_stats (admitted / skipped keep adding up over several counts) last until prefilter_create or _free.
 * TSX_HIP_EINVAL, before any GPU call: bits outside 12 .. 38; add, arm(1) or read without a filter; an armed count on a
 *   map created with shard_bits > 0 or on a table that is built slab by slab (above 2^32 slots); armed wrapped-FASTA
 *   counting (tsx_hip_count_fasta_*); a device text that is not 16-byte aligned; tsx_hip_group_count_fastq_host while
 *   a map of the group is armed (each GPU sees a share of the records only).
 *   prefilter_create    allocates and zeroes A (2^bits / 8 bytes) and B (a quarter), zeroes the totals, disarms.  A second
 *                       call replaces them.  prefilter_free releases them and disarms.
 *   prefilter_add_host  pass 1 over a text in host memory, in pieces cut at record boundaries (chunk_bytes 0 = 256 MiB,
 *                       and at most TSX_HIP_PIECE_BYTES when that is set).  _add_bgzf_host: the image of a BGZF file.
 *   prefilter_add_device  dev_text as tsx_hip_sketch_device takes it; queued on the stream, not waited for.
 *   prefilter_arm       on != 0: the FASTQ counting calls run pass 2 until it is taken back.
 *   prefilter_stats     bits; seen = windows of pass 1; seen_again = those that found their k-mer in A (or in the lane
 *                       below); admitted / skipped = windows of pass 2 that were inserted / kept out; set_bits_a / _b =
 *                       the filters' fill.  Without a filter: all zero.
 *   prefilter_read      which = 0: A, 1: B; nwords must be the filter's 2^(bits - 6) / 2^(bits - 8) (else TSX_HIP_ERANGE).
 *   prefilter_mask_host CPU only, the definition: word indexes and mask of ONE k-mer as given (the caller canonicalises).
 */
typedef struct tsx_hip_prefilter_totals {
    uint64_t bits, seen, seen_again, admitted, skipped, set_bits_a, set_bits_b;
} tsx_hip_prefilter_totals;
int tsx_hip_prefilter_create(tsx_hip_map *m, int bits);
int tsx_hip_prefilter_free(tsx_hip_map *m);
int tsx_hip_prefilter_add_host(tsx_hip_map *m, const char *text, size_t n, size_t chunk_bytes);
int tsx_hip_prefilter_add_bgzf_host(tsx_hip_map *m, const void *gz, size_t n);
int tsx_hip_prefilter_add_device(tsx_hip_map *m, const void *dev_text, size_t n, void *stream);
int tsx_hip_prefilter_arm(tsx_hip_map *m, int on);
int tsx_hip_prefilter_armed(const tsx_hip_map *m);   /* 1 or 0 */
int tsx_hip_prefilter_bits(const tsx_hip_map *m);    /* the bits of the map's filter, 0 without one; host state, no GPU call */
int tsx_hip_prefilter_stats(tsx_hip_map *m, tsx_hip_prefilter_totals *out);
int tsx_hip_prefilter_read(tsx_hip_map *m, int which, uint64_t *words_out, size_t nwords);
int tsx_hip_prefilter_mask_host(int k, const uint64_t *kmer_limbs, int bits, uint64_t *word_a, uint64_t *word_b,
                                uint64_t *mask);

/*
 * Paired reads kept in step (csrc/tsx_pairs.h; no reference counterpart -- khmer `--paired`, Trimmomatic PE, BBDuk
 * in1/in2): the filter and the trim over mate pairs, so that the outputs line up record for record.  Records, lines,
 * k-mers, c(x) and the base rule are those of tsx_hip_query_reads_*.
 *   Two texts A and B (text2 != NULL): pair i is record i of A (mate 1) and record i of B (mate 2).  Record counts are
 *     as tsx_hip_query_reads_host reports them (a trailing incomplete record is one record).
 *   One interleaved text (text2 == NULL, n2 = 0): pair i is records 2 i and 2 i + 1.
 * Different record counts in A and B, or an odd count in an interleaved text: TSX_HIP_EPAIR.
 * check_names != 0: the NAME of a record is the part of its first line after the first byte ('@' or '>') up to the
 *   first space or tab, or the line's end, with one trailing "/1" or "/2" removed.  Mates must have byte-equal names; the
 *   first pair that does not gives TSX_HIP_EPAIR, and tsx_hip_last_error names the pair's index (from 0).  The names are
 *   compared on the device.  check_names == 0: names are not looked at.
 * On TSX_HIP_EPAIR the outputs hold, at most, whole pairs from the pieces before the one that failed.
 * Filter: a mate's verdict is that of tsx_hip_filter_reads_* under the same rule, invert included.  pair_mode
 *   TSX_HIP_PAIR_BOTH keeps a pair when both verdicts hold, TSX_HIP_PAIR_ANY when at least one does.  A kept pair writes
 *   both mates whole, by the filter's write rules (the '\n' added for an unterminated last line of either text; empty
 *   lines are not written).  Under BOTH a mate that passes while its partner fails is an ORPHAN; ANY has no orphans.
 * Trim: each mate is trimmed on its own by the rule.  A mate SURVIVES when tsx_hip_trim_reads_* would write it (length
 *   >= min_len, 0 = k).  A pair is kept when both survive, each mate written exactly as the single-end trim writes it; a
 *   lone survivor is an orphan, written the same way.
 * Outputs (tsx_hip_pair_io), everything in input order:
 *   two texts    kept mates 1 to fd1, kept mates 2 to fd2 (both required); orphans of A to fd_single1, of B to
 *                fd_single2 (each may be -1: those orphans are dropped, and still counted)
 *   interleaved  kept pairs to fd1 as mate 1, mate 2; orphans to fd_single1 (may be -1); fd2 and fd_single2 must be -1
 * totals (optional): pairs seen, pairs kept, orphans of each side (mate 1 / mate 2 for an interleaved text), bytes
 * written per output (0 for a dropped one); for the trim also bases_in = bases of all sequence lines seen and
 * bases_kept = bases of the kept pairs and the orphans (dropped orphans included); the filter leaves both 0.
 * The texts are taken in pieces of chunk_bytes each (0 = 256 MiB; a record longer than a piece is taken whole); every
 * round takes the same number of records from both; the device works on round i + 1 while the host writes round i.
 * TSX_HIP_EINVAL, before any HIP call: what the single-end calls refuse (a map created with shard_bits > 0, lower >
 * upper, fraction_ppm > 10^6, an unknown trim mode, reserved != 0), an unknown pair_mode, io == NULL, a required fd < 0,
 * an fd that must be -1 and is not.  A failed write: TSX_HIP_EIO.
 */
#define TSX_HIP_PAIR_BOTH 0
#define TSX_HIP_PAIR_ANY 1
typedef struct tsx_hip_pair_io {
    int fd1, fd2, fd_single1, fd_single2;
} tsx_hip_pair_io;
typedef struct tsx_hip_pair_totals {
    uint64_t pairs, kept, single1, single2;
    uint64_t bytes1, bytes2, bytes_single1, bytes_single2;
    uint64_t bases_in, bases_kept;
} tsx_hip_pair_totals;
int tsx_hip_filter_pairs_host(tsx_hip_map *m, const char *text1, size_t n1, const char *text2, size_t n2,
                              const tsx_hip_filter_rule *rule, int pair_mode, int check_names, const tsx_hip_pair_io *io,
                              size_t chunk_bytes, tsx_hip_pair_totals *totals);
int tsx_hip_trim_pairs_host(tsx_hip_map *m, const char *text1, size_t n1, const char *text2, size_t n2,
                            const tsx_hip_trim_rule *rule, int check_names, const tsx_hip_pair_io *io, size_t chunk_bytes,
                            tsx_hip_pair_totals *totals);

/*
 * Table set operations (csrc/tsx_combine.h; no reference counterpart -- `kmc_tools simple`, `jellyfish merge --min/--max`):
 * the k-mers of two tables A and B joined on the device into an EMPTY third table OUT, or only compared.  a(x), b(x) are
 * getKmerCount(x) in A and B (in-slot field plus carries, 0 when absent; on canonical tables x is the pair).  First the
 * ranges: a'(x) = a(x) if a_lower <= a(x) <= a_upper, else 0; the same for b'.  Then
 *   op         x is in OUT iff        its count
 *   INTERSECT  a' > 0 and b' > 0      MIN: min(a', b'); MAX: max; SUM: a' + b' (mod 2^64); LEFT: a'; RIGHT: b'
 *   UNION      a' > 0 or b' > 0       both present: as INTERSECT; one present: that one's count (every count mode)
 *   SUBTRACT   a' > 0 and b' = 0      a' (count_mode ignored)
 *   DIFF       a' > b'                a' - b' (count_mode ignored)
 * A lower bound of 0 is taken as 1 (an absent k-mer is never in range).  UNION / SUM with full ranges gives the table
 * that tsx_hip_load_host gives when it merges B's database into A.
 *   out == NULL   nothing is written, only stats_out is filled (Jaccard index = both / (a_in_range + b_in_range - both));
 *                 out_entries / out_count_sum are then what the rule WOULD write.
 *   out           empty (just created or after tsx_hip_clear), not a and not b, on the same device.  a == b is allowed.
 * All three agree in k, canonical mode and base rule, and none was created with shard_bits > 0; l, storage bits,
 * overflow_l and hash seed may differ between all three.  A and B are left as they are, bit for bit.  OUT's kmers_added
 * grows by out_count_sum (count_sum == kmers_added keeps holding), its distinct is out_entries.  The call waits for what
 * is queued on the three maps' streams, and for its own result.
 * Two paths with identical results: when A and B share l, slot layout, segment bits and seed (the condition of
 * tsx_hip_load_host's direct placement) the join works on hashed keys and stays inside one table segment per key
 * ("aligned"; with OUT of that geometry too, nothing is staged); any other pair goes through k-mers ("general").
 * TSX_HIP_EINVAL (tsx_hip_last_error says which): lower > upper, an unknown op or count mode, out not empty or equal to
 * a or b, maps on different devices, a different k, canonical mode or base rule, a map created with shard_bits > 0.
 * TSX_HIP_EFULL: a k-mer did not fit into OUT (sticky as for inserts; OUT's content is then unspecified, tsx_hip_clear
 * recovers it).  TSX_HIP_EOVERFLOW: OUT's secondary array is full.
 */
enum { TSX_HIP_OP_INTERSECT = 0, TSX_HIP_OP_UNION = 1, TSX_HIP_OP_SUBTRACT = 2, TSX_HIP_OP_DIFF = 3 };
enum { TSX_HIP_CNT_MIN = 0, TSX_HIP_CNT_MAX = 1, TSX_HIP_CNT_SUM = 2, TSX_HIP_CNT_LEFT = 3, TSX_HIP_CNT_RIGHT = 4 };
typedef struct tsx_hip_combine_rule {
    int32_t op, count_mode;
    uint64_t a_lower, a_upper, b_lower, b_upper;   /* the count range of each input (kmc_tools -ci / -cx) */
} tsx_hip_combine_rule;
typedef struct tsx_hip_combine_stats {
    uint64_t a_in_range, b_in_range;   /* distinct k-mers of A / B whose count is in its range */
    uint64_t both;                     /* distinct k-mers in range in both */
    uint64_t a_sum_both, b_sum_both;   /* sum of a' / b' over those */
    uint64_t out_entries, out_count_sum;
} tsx_hip_combine_stats;
int tsx_hip_combine(tsx_hip_map *out, tsx_hip_map *a, tsx_hip_map *b, const tsx_hip_combine_rule *rule,
                    tsx_hip_combine_stats *stats_out /* optional */);

/*
 * Joint k-mer spectrum of two tables (csrc/tsx_joint.h; no reference counterpart -- KAT `comp`, the spectra-cn matrix):
 * how many distinct k-mers occur i times in A and j times in B, for every pair (i, j), binned on the device.
 *   A, B     two whole tables (none created with shard_bits > 0) on one device that agree in k, canonical mode and base
 *            rule; l, storage bits, overflow_l and hash seed may differ (the conditions of tsx_hip_combine).  a == b is
 *            allowed.
 *   a(x)     getKmerCount(x) in A, b(x) in B: in-slot field plus carries from the secondary array, 0 when x is absent;
 *            on canonical tables x stands for its strand pair, as in tsx_hip_combine.
 *   bins     na, nb >= 2; bin_a(c) = min(c, na - 1), bin_b(c) = min(c, nb - 1): the last bin of each side pools every
 *            larger count, as tsx_hip_histogram_* does.  na * nb <= 2^24.
 *   matrix   uint64, row-major, na x nb: M[i * nb + j] = the number of distinct x in A u B (a(x) > 0 or b(x) > 0) with
 *            bin_a(a(x)) = i and bin_b(b(x)) = j.  M[0] = 0.  Row 0 is what only B holds, column 0 what only A holds;
 *            the sums of rows i >= 1 are A's abundance histogram, the sums of columns j >= 1 are B's.  There are no
 *            count ranges: a range is a sum over cells.
 *   _device  zeroes dev_matrix (na * nb * 8 bytes, device memory), waits for what is queued on both maps' streams, and
 *            queues the sweeps on `stream` (NULL = A's own): it returns without waiting for them.  What A's and B's own
 *            streams do next is ordered behind them.
 *   _host    the same into host memory; waits for the result.
 * A and B are left as they are, bit for bit (a lazily cleared table is zeroed first, as everywhere).  The two paths of
 * tsx_hip_combine apply, with identical results, and TSX_HIP_COMBINE_PATH picks one in the same way.
 * TSX_HIP_EINVAL (tsx_hip_last_error says which): a NULL map or matrix, a map created with shard_bits > 0, maps on
 * different devices, a different k, canonical mode or base rule, na < 2, nb < 2, na * nb > 2^24, a forced path that does
 * not apply.
 */
int tsx_hip_joint_histogram_device(tsx_hip_map *a, tsx_hip_map *b, size_t na, size_t nb, void *dev_matrix, void *stream);
int tsx_hip_joint_histogram_host(tsx_hip_map *a, tsx_hip_map *b, uint64_t *matrix_out, size_t na, size_t nb);

/*
 * Read binning by two tables (csrc/tsx_bin.h; no reference counterpart -- trio binning with hapmers as Canu and Merqury
 * do it, BBSplit, xenograft sorting): ONE scan of a text against two tables, per record the windows that hit A and the
 * windows that hit B, and from those the table the record belongs to.  Records, lines, k-mers, the stand-in code,
 * canonical keys and the base rule are those of tsx_hip_query_reads_*.
 *   A, B     two whole tables (none created with shard_bits > 0) on one device that agree in k, canonical mode and base
 *            rule; l, storage bits, overflow_l and hash seed may differ (the conditions of tsx_hip_combine).  a == b is
 *            allowed.  a(x) and b(x) are getKmerCount(x) in A and in B, carries from the secondary array included, 0
 *            when x is absent.
 *   stats    per record (tsx_hip_bin_stats): kmers as in tsx_hip_read_stats (under a base rule only the windows that are
 *            k-mers); hits_a = the windows with a_lower <= a(x) <= a_upper, with multiplicity; hits_b the same for B
 *            with b_lower .. b_upper; hits_both = the windows in range in both.  A lower bound of 0 is taken as 1, as
 *            in tsx_hip_combine.
 *   rule     qa = hits_a >= min_hits, qb = hits_b >= min_hits;
 *            wins_a = qa && hits_a > hits_b && hits_a * 1000 >= ratio_milli * hits_b, wins_b its mirror image;
 *            1000 <= ratio_milli <= 1000000 (the products fit 64 bits: a sequence line is shorter than 4 GiB).
 *            min_hits = 1 and ratio_milli = 1000 are the plain rule: more hits wins, ties win nothing.
 *   class    TSX_HIP_BIN_A if wins_a, TSX_HIP_BIN_B if wins_b (they cannot hold together), TSX_HIP_BIN_NONE if neither qa
 *            nor qb, TSX_HIP_BIN_AMBIGUOUS otherwise.  A record without k-mers is NONE when min_hits >= 1; min_hits = 0
 *            is legal and makes every record at least AMBIGUOUS.
 *   output   tsx_hip_bin_io names one file descriptor per class; -1 counts the class and writes nothing.  A written
 *            record is its bytes exactly as tsx_hip_filter_reads_* writes a kept record (the added '\n' included, empty
 *            lines not written).  Every output is in input order; every record lands in exactly one class.
 *   totals   records, n[class], bytes[class] (0 for a dropped output).
 *   bin_stats_device  dev_text as tsx_hip_query_reads_device takes it; the stats of records [0, stats_cap) to dev_stats
 *                     (zeroed by the call), queued on `stream` (NULL = A's own).  WAITS and reports the record count;
 *                     more records than stats_cap: TSX_HIP_ERANGE (the first stats_cap are written).
 *   bin_stats_host    text in host memory, in pieces as tsx_hip_query_reads_host (chunk_bytes, 0 = 256 MiB); stats_out
 *                     and, when class_out is not NULL, one class byte per record, for records [0, stats_cap).
 *   bin_reads_host    the same pieces; the device compacts the outputs of a piece while the host writes those of the
 *                     piece before.  A failed write: TSX_HIP_EIO.
 * The calls wait for what is queued on both maps' own streams before they start.  A and B are left as they are, bit for
 * bit (a lazily cleared table is zeroed first, as everywhere).
 * TSX_HIP_EINVAL before any device call (tsx_hip_last_error says which): a NULL rule, lower > upper on either side,
 * ratio_milli outside 1000 .. 10^6, reserved != 0, io == NULL or every fd of io equal to -1, a NULL map, a map created
 * with shard_bits > 0, maps on different devices, a different k, canonical mode or base rule.
 */
enum { TSX_HIP_BIN_A = 0, TSX_HIP_BIN_B = 1, TSX_HIP_BIN_AMBIGUOUS = 2, TSX_HIP_BIN_NONE = 3 };
typedef struct tsx_hip_bin_stats {
    uint64_t kmers, hits_a, hits_b, hits_both;
} tsx_hip_bin_stats;
typedef struct tsx_hip_bin_rule {
    uint64_t a_lower, a_upper;   /* the count range of a hit in A */
    uint64_t b_lower, b_upper;   /* ... in B */
    uint64_t min_hits;           /* hits a side needs to qualify */
    uint32_t ratio_milli;        /* the winner's hits are at least this many thousandths of the loser's */
    int32_t reserved;            /* 0 */
} tsx_hip_bin_rule;
typedef struct tsx_hip_bin_io {
    int fd_a, fd_b, fd_ambiguous, fd_none;
} tsx_hip_bin_io;
typedef struct tsx_hip_bin_totals {
    uint64_t records, n[4], bytes[4];   /* n and bytes by class */
} tsx_hip_bin_totals;
int tsx_hip_bin_stats_device(tsx_hip_map *a, tsx_hip_map *b, const void *dev_text, size_t n, const tsx_hip_bin_rule *rule,
                             void *dev_stats, size_t stats_cap, size_t *n_records, void *stream);
int tsx_hip_bin_stats_host(tsx_hip_map *a, tsx_hip_map *b, const char *text, size_t n, const tsx_hip_bin_rule *rule,
                           tsx_hip_bin_stats *stats_out, uint8_t *class_out /* optional, one byte per record */,
                           size_t stats_cap, size_t *n_records, size_t chunk_bytes);
int tsx_hip_bin_reads_host(tsx_hip_map *a, tsx_hip_map *b, const char *text, size_t n, const tsx_hip_bin_rule *rule,
                           const tsx_hip_bin_io *io, size_t chunk_bytes, tsx_hip_bin_totals *totals /* optional */);

/*
 * Heterozygous k-mer pairs of one table (csrc/tsx_het.h; no reference counterpart -- Smudgeplot's `hetkmers`): the pairs
 * of k-mers of the table that differ only in their middle base, by the two counts of each pair.
 *   c(x)      getKmerCount(x): in-slot field plus carries, as tsx_hip_joint_histogram_* reads it.  x is in range when
 *             rule->lower <= c(x) <= rule->upper; a k-mer out of range counts as absent everywhere below (the a_range
 *             convention of tsx_hip_combine).
 *   middle    base p = (k - 1) / 2: bits 2p, 2p + 1 of the tsx_hip_encode layout, limb p / 32.  k must be odd (so that the
 *             middle base stays the middle base under reverse complement and the relation is symmetric).
 *   family    of x: the in-range table keys among x and its three middle-base variants; on a canonical table every variant
 *             is taken to its strand pair's key first, and duplicates are dropped (flanks that are reverse complements of
 *             each other, AC?GT, have only two keys: A/T in the middle and C/G).
 *   pair      an unordered set of two distinct members of one family.  mode 0 (unique, Smudgeplot's rule) counts a pair
 *             only when its family has exactly two members; mode 1 (all) counts every pair of every family, up to 6 per
 *             family.  Each pair is counted once.
 *   matrix    uint64, row-major, n_minor x n_major, n_minor, n_major >= 2, n_minor * n_major <= 2^24:
 *             M[min(cmin, n_minor - 1) * n_major + min(cmax, n_major - 1)] = the pairs {x, y} with cmin = min(c(x), c(y))
 *             and cmax = max(c(x), c(y)).
 *   stats     kmers_in_range; paired = k-mers in at least one counted pair; pairs; families_2 / families_3plus = families
 *             of exactly 2 / of 3 or 4 members, each counted once whatever the mode.
 *   record    of the pair list: 2 * key_limbs + 2 uint64 -- minor k-mer (key_limbs words, tsx_hip_encode layout), major
 *             k-mer, minor count, major count.  Minor is the lower count, on a tie the k-mer whose text is smaller.  K-mers
 *             are reported as dumps report them (canonical tables: the smaller strand).  The order is unspecified.
 *   _histogram_device  zeroes dev_matrix (n_minor * n_major * 8 bytes) and dev_stats (sizeof(tsx_hip_het_stats), both device
 *             memory), waits for what is queued on the map's stream and queues the sweep on `stream` (NULL = the map's
 *             own): it returns without waiting for it.
 *   _histogram_host    the same into host memory (stats_out optional); waits for the result.
 *   _pairs_device      the pairs owned by slots [slot_lo, slot_hi) -- every pair is owned by exactly one slot, so that
 *             disjoint ranges that cover the table give every pair once -- into dev_pairs (cap records); *dev_n (uint64,
 *             device) receives their number.  Waits for the result; more pairs than cap: TSX_HIP_ERANGE, the first cap
 *             records are written and *dev_n is the true total.  S slots own at most S pairs in mode 0, 3 S in mode 1.
 *   tsx_hip_write_het_pairs_host  the list as text, minor_kmer<TAB>minor_count<TAB>major_kmer<TAB>major_count per line, to
 *             fd, chunk by chunk (the device makes chunk i + 1 while the host writes chunk i).  chunk_bytes bounds the text
 *             of a chunk (0 = 256 MiB); a chunk is at least 64 slots, less room than that is TSX_HIP_EINVAL.
 * The table is left as it is, bit for bit (a lazily cleared table is zeroed first, as everywhere).
 * TSX_HIP_EINVAL before any device call (tsx_hip_last_error says which): a NULL map, rule or output, even k, a map created
 * with shard_bits > 0, lower > upper, an unknown mode, reserved != 0, fewer than 2 bins on a side, more than 2^24 cells,
 * slot_lo > slot_hi or a range beyond the table.
 */
#define TSX_HIP_HET_UNIQUE 0
#define TSX_HIP_HET_ALL 1
typedef struct tsx_hip_het_rule {
    uint64_t lower, upper;
    int32_t mode;       /* TSX_HIP_HET_UNIQUE or TSX_HIP_HET_ALL */
    int32_t reserved;   /* 0 */
} tsx_hip_het_rule;
typedef struct tsx_hip_het_stats {
    uint64_t kmers_in_range, paired, pairs, families_2, families_3plus;
} tsx_hip_het_stats;
int tsx_hip_het_histogram_device(tsx_hip_map *m, const tsx_hip_het_rule *rule, size_t n_minor, size_t n_major, void *dev_matrix,
                                 void *dev_stats, void *stream);
int tsx_hip_het_histogram_host(tsx_hip_map *m, const tsx_hip_het_rule *rule, uint64_t *matrix_out, size_t n_minor, size_t n_major,
                               tsx_hip_het_stats *stats_out /* optional */);
int tsx_hip_het_pairs_device(tsx_hip_map *m, const tsx_hip_het_rule *rule, uint64_t slot_lo, uint64_t slot_hi, void *dev_pairs,
                             size_t cap, void *dev_n, void *stream);
int tsx_hip_write_het_pairs_host(tsx_hip_map *m, const tsx_hip_het_rule *rule, int fd, size_t chunk_bytes, uint64_t *pairs_out,
                                 uint64_t *bytes_out);

/*
 * Unitigs: the compacted de Bruijn graph of one table (csrc/tsx_unitig.h; no reference counterpart -- BCALM2, Cuttlefish).
 *   node      a k-mer x of the table with rule->lower <= c(x) <= rule->upper (c as above); a k-mer out of range is absent.
 *             On a canonical table a node stands for both strands.
 *   oriented  a node read as a string s: on a canonical table a node has two, s and rc(s), on a plain table one.  succ(s)
 *             is the set of strings s[1:] + c, c in ACGT, that are nodes (either strand, on a canonical table), pred(s) the
 *             set of strings c + s[:-1] that are.
 *   edge      s -> t, t in succ(s), is compactable when |succ(s)| = 1, |pred(t)| = 1 and t is not the node of s (no
 *             AAAA -> AAAA, no hairpin s -> rc(s)).
 *   unitig    a maximal chain s1 -> ... -> sm of compactable edges, spelled as s1 followed by the last base of each later
 *             string: m + k - 1 bases that hold m k-mers.  On a canonical table every chain exists on both strands and the
 *             lexicographically smaller spelling is reported; k must be odd there (no k-mer is its own reverse
 *             complement, so a chain never meets a node twice).  A chain that closes on itself -- an isolated cycle -- is cut
 *             at a node of the library's choice, spelled the same way and marked circular; its strand is free as well.
 *             Every node lies in exactly one unitig, once; the set of unitigs depends on the node set alone.
 *   record    tsx_hip_unitig: the sequence is bytes [offset, offset + length) of the sequence buffer (ASCII, no separator;
 *             the records tile the buffer in no particular order), kmers = m, sum_count = the exact sum of the m counts
 *             (modulo 2^64).  The order of the records is unspecified.
 *   totals    nodes; unitigs; circular; bases = the sum of the lengths; longest = the most bases of one unitig; isolated =
 *             nodes without any neighbour; tips = nodes with neighbours on one side only; branching = nodes with more than
 *             one neighbour on a side; sum_count over all nodes; degree[5 * in + out] = nodes by |pred| and |succ| of the
 *             strand a dump reports.
 *   tsx_hip_unitig_stats     the totals alone: the degree sweep and the walks, nothing spelled.
 *   tsx_hip_unitigs_device   sequences to dev_seq (seq_cap bytes) and records to dev_records (record_cap records), both device
 *                            memory, on `stream` (NULL = the map's own).  WAITS for the result.  *n_unitigs and *seq_bytes
 *                            always receive what the result needs; a cap below that: TSX_HIP_ERANGE, and neither buffer
 *                            holds anything of use (nothing is written past the caps).
 *   tsx_hip_unitigs_host     the same into host memory.
 *   tsx_hip_write_unitigs_host  FASTA to fd, one record per unitig with BCALM's header, `>INDEX LN:i:<bases> KC:i:<sum_count>
 *                            km:f:<sum_count / kmers as %.1f>`, ` CL:i:1` behind it for a circular one, the sequence on one
 *                            line.  Written chunk by chunk behind the copies from the device.  A failed write: TSX_HIP_EIO.
 * Extra device memory for the length of a call: one byte and one bit per slot, 8 bytes per unitig, and for the _host and
 * write calls the records (40 bytes each) and the sequences; the record room of those two is min(record_cap, nodes), and
 * when that passes 256 MiB the walks run once more, in front, so that it is the unitigs.  TSX_HIP_ENOMEM when it does not
 * fit.  The table is left as it is.
 * TSX_HIP_EINVAL before any device call (tsx_hip_last_error says which): a NULL map, rule or output, a map created with
 * shard_bits > 0, lower > upper, flags or reserved != 0, even k on a canonical table.  TSX_HIP_EHIP with "unitigs: the table
 * is not consistent" when a walk ran into its bound of nodes + 1 steps (no device loop depends on the table to end).
 */
typedef struct tsx_hip_unitig_rule {
    uint64_t lower, upper;
    uint32_t flags;      /* 0 */
    uint32_t reserved;   /* 0 */
} tsx_hip_unitig_rule;
typedef struct tsx_hip_unitig {
    uint64_t offset, length, kmers, sum_count, circular;
} tsx_hip_unitig;
typedef struct tsx_hip_unitig_totals {
    uint64_t nodes, unitigs, circular, bases, longest, isolated, tips, branching, sum_count;
    uint64_t degree[25];
} tsx_hip_unitig_totals;
int tsx_hip_unitig_stats(tsx_hip_map *m, const tsx_hip_unitig_rule *rule, tsx_hip_unitig_totals *totals);
int tsx_hip_unitigs_device(tsx_hip_map *m, const tsx_hip_unitig_rule *rule, void *dev_seq, size_t seq_cap, void *dev_records,
                           size_t record_cap, size_t *n_unitigs, size_t *seq_bytes, tsx_hip_unitig_totals *totals /* optional */,
                           void *stream);
int tsx_hip_unitigs_host(tsx_hip_map *m, const tsx_hip_unitig_rule *rule, void *seq_out, size_t seq_cap,
                         tsx_hip_unitig *records_out, size_t record_cap, size_t *n_unitigs, size_t *seq_bytes,
                         tsx_hip_unitig_totals *totals /* optional */);
int tsx_hip_write_unitigs_host(tsx_hip_map *m, const tsx_hip_unitig_rule *rule, int fd, tsx_hip_unitig_totals *totals /* optional */);
/* A DIAGNOSTIC for scripts/unitig_rate.py, with no promise of stability: it may change or go in any release.  What the
 * steps of this thread's last unitig call took, in milliseconds of host clock (every step waits for its totals):
 * ms_out[0] the degree sweep, [1] the walk of the starts (both of them when the walks ran twice), [2] the spelling walk,
 * [3] the cycle pass. */
int tsx_hip_unitig_last_timing(double *ms_out);

/* IBijectiveFunction::apply / inv_apply (IBijectiveFunction.h:26-27) on the host,
 * and the matrix rows (row i <-> output bit 2k-1-i, BijectiveKMapping.h:202-256). */
int tsx_hip_hash_apply(const tsx_hip_map *m, const uint64_t *kmer, uint64_t *key_out);
int tsx_hip_hash_invert(const tsx_hip_map *m, const uint64_t *key, uint64_t *kmer_out);
int tsx_hip_hash_rows(const tsx_hip_map *m, uint64_t *rows_out /* 2k x key_limbs */);
/* One-limb keys (k <= 32): the 16 x 16 table by 4-bit groups that the walk hashes a strip's first window with, as a map
 * made with (k, l, hash_seed) gets it: lut_out[grp * 16 + v] = M * ((v << 4 grp) & (2^2k - 1)).  Host only, no GPU call. */
int tsx_hip_lut4_host(int k, int l, uint64_t hash_seed, uint64_t *lut_out /* 256 */);
/* The level-1 sub-lists of the partitioned path (walk fused with radix level 1): list (b, g) -- bucket b of nb, walk
 * workgroup g of G -- holds at most cap records and starts at record tsx_hip_sublist_first() of its buffer, numbered
 * bucket-major (b * G + g) or, after a plain one-GPU count, workgroup-major (g * nb + b); its size is published at the
 * same number.  tsx_hip_level1_sizes_host: shape and order of the lists the LAST such count of the map left and, with
 * sizes_out (room for nb * G), their published sizes in that order -- valid until the map counts again.  For tests. */
typedef struct tsx_hip_level1_shape {
    uint32_t nb, G, cpr2;   /* cpr2: level-2 workgroups per bucket; workgroup c reads pieces c, c + cpr2, ... as one stream */
    int wg_major;
    uint64_t cap;
} tsx_hip_level1_shape;
uint64_t tsx_hip_sublist_first(uint32_t nb, uint32_t G, int wg_major, uint32_t b, uint32_t g, uint64_t cap);
int tsx_hip_level1_sizes_host(tsx_hip_map *m, tsx_hip_level1_shape *shape_out, uint64_t *sizes_out /* optional */, size_t cap);

/*
 * Multi-GPU counting with a sharded table (k <= 32).  Reads shard across the GPUs;
 * what travels between them is hashed keys BEFORE they are built into a table, not
 * table slots afterwards:
 *   shard_scan_window_device  scans the window [win_off, win_off + win_len) of this GPU's
 *                       device text (n_total bytes; win_off a multiple of 16; windows of one
 *                       text are given in order, win_off == 0 restarts the line count, a
 *                       window may begin anywhere -- inside a line, inside a record) and writes
 *                       the hashed keys of all its k-mers grouped by owner GPU into dev_send
 *                       (capacity from tsx_hip_shard_send_capacity(win_len)):
 *                       dev_send_counts[o] = keys for owner o.  With dev_own != NULL the keys
 *                       this GPU owns go there instead (they never travel) and dev_send holds
 *                       the other owners' groups back to back.  Keys that carry a count (hot
 *                       k-mers merged on chip) go to the (dev_hot_keys, dev_hot_counts) list,
 *                       *dev_hot_n of them.  *dev_key_sum (optional) += sum of all keys
 *                       written (mod 2^64): the integrity check of the exchange.
 *   shard_scan_device   the same for a whole text as one window, own keys inside dev_send.
 *   -- all-to-all of the owner groups (RCCL), all-gather of the hot lists --
 *   shard_build_device  builds the received keys into this GPU's slot range (radix
 *                       partition + LDS segment build); *dev_key_sum (optional) += their sum.
 *                       shard_build_pieces_device: the same for several runs of keys at once.
 *   add_hashed_device   adds (hashed key, count) pairs, skipping other owners' keys.
 * tsxcount_amd/distributed.py: ShardedCounter.
 */
int tsx_hip_shard_send_capacity(tsx_hip_map *m, size_t text_bytes, size_t *keys_out);
int tsx_hip_shard_scan_window_device(tsx_hip_map *m, const void *dev_text, size_t n_total, size_t win_off,
                                     size_t win_len, void *dev_send, size_t send_cap_keys, void *dev_own,
                                     size_t own_cap_keys, void *dev_send_counts, void *dev_hot_keys,
                                     void *dev_hot_counts, size_t hot_cap, void *dev_hot_n, void *dev_key_sum,
                                     void *stream);
int tsx_hip_shard_scan_device(tsx_hip_map *m, const void *dev_text, size_t n, void *dev_send,
                              size_t send_cap_keys, void *dev_send_counts, void *dev_hot_keys,
                              void *dev_hot_counts, size_t hot_cap, void *dev_hot_n, void *stream);
int tsx_hip_shard_build_device(tsx_hip_map *m, const void *dev_keys, size_t n_keys, void *dev_key_sum,
                               void *stream);
/* The same for keys that arrived in several runs (own keys and one run per exchange window): run i is
 * piece_cnt[i] keys at dev_keys + piece_off[i] (host arrays, in keys).  ONE partition + build for all of
 * them: a build costs a full pass over this GPU's slot range however few keys it brings. */
int tsx_hip_shard_build_pieces_device(tsx_hip_map *m, const void *dev_keys, const uint64_t *piece_off,
                                      const uint64_t *piece_cnt, size_t npieces, void *dev_key_sum, void *stream);
/* Level 1 window by window.  tsx_hip_shard_l1_window_device partitions the n_keys received keys of exchange
 * window `window` (of nwindows) by radix level 1 as soon as they have arrived -- the later windows are still being
 * exchanged -- into sub-lists of its own (window 0 plans for est_total_keys keys in all; more than that is not an
 * error, only slower).  tsx_hip_shard_build_l1_device then runs level 2 + the build over what the windows left:
 * only these two wait for the last window.  tsx_hip_shard_l1_supported: one-limb keys and a table split by two
 * radix levels (otherwise: tsx_hip_shard_build_pieces_device). */
int tsx_hip_shard_l1_supported(tsx_hip_map *m);
int tsx_hip_shard_l1_window_device(tsx_hip_map *m, const void *dev_keys, size_t n_keys, uint32_t window, uint32_t nwindows,
                                   size_t est_total_keys, void *dev_key_sum, void *stream);
int tsx_hip_shard_build_l1_device(tsx_hip_map *m, void *stream);

/* Description exchange (small world sizes).  A strip description (16 bytes: 48 bases as 2-bit codes + 16 validity
 * bits) stands for up to 16 k-mer occurrences, a key for one: instead of sending every key to its owner, every GPU
 * describes its text window (tsx_hip_shard_desc_window_device: dev_count[0] packed descriptions at dev_desc,
 * dev_kmer_sum += k-mer occurrences they stand for), the
 * descriptions are all-gathered, and every GPU walks all of them and keeps the keys it owns
 * (tsx_hip_shard_walk_device, one call per (window, source GPU) = slot of nslots; slot 0 plans for est_total_keys owned
 * keys; dev_emit_sum += k-mer occurrences kept -- over all GPUs that must equal the k-mers scanned).  N x the rolling
 * work for N/8 of the bytes on the wire.  long_desc: four neighbouring strips in one description of 32 bytes (96 bases +
 * 64 validity bits) -- half the bytes again; dev_desc / desc_cap / n_desc then count those.  Then
 * tsx_hip_shard_build_l1_device.  Same support as tsx_hip_shard_l1_supported. */
int tsx_hip_shard_desc_capacity(tsx_hip_map *m, size_t text_bytes, int long_desc, size_t *descs_out);
int tsx_hip_shard_desc_window_device(tsx_hip_map *m, const void *dev_text, size_t n_total, size_t win_off, size_t win_len,
                                     int long_desc, void *dev_desc, size_t desc_cap, void *dev_count, void *dev_kmer_sum,
                                     void *stream);
int tsx_hip_shard_walk_device(tsx_hip_map *m, const void *dev_desc, size_t n_desc, int long_desc, uint32_t slot,
                              uint32_t nslots, size_t est_total_keys, void *dev_emit_sum, void *stream);
/* The same result in two kernels (owner-filtered walk into per-wave key logs, then radix level 1 over the logs): the
 * better form when this GPU keeps few of the keys it walks (world sizes >= 4). */
int tsx_hip_shard_filter_device(tsx_hip_map *m, const void *dev_desc, size_t n_desc, int long_desc, uint32_t slot,
                                uint32_t nslots, size_t est_total_keys, void *dev_emit_sum, void *stream);

int tsx_hip_add_hashed_device(tsx_hip_map *m, const void *dev_keys, const void *dev_counts, size_t n,
                              void *stream);

/* Minimizer exchange (any world size <= 16, 20 <= k <= 32; csrc/tsx_minimizer.h).  The owner of a k-mer is a function of
 * its minimizer (the m-mer with the smallest hash value, m = min(11, k - 15)), so runs of consecutive k-mers share an owner
 * and every GPU holds a WHOLE table (shard_bits = 0) of the k-mers it owns: no slot-range split, no merge, and nobody walks
 * a position it does not own.  tsx_hip_mini_window_device describes a text window and splits the strip descriptions by
 * owner: list o (packed, dev_counts[o] descriptions, a multiple of 64 -- holes carry no valid start) at
 * dev_desc + o * cap_per_owner * 16 bytes, cap_per_owner >= tsx_hip_mini_capacity(win_len); dev_counts[nranks + b] =
 * occurrences of the homopolymer k-mer of base b (A, C, G, T) in the window, which are NOT in the descriptions: the caller
 * adds the totals on the owner of each (tsx_hip_mini_owner_host, tsx_hip_add_kmers_device); dev_kmer_sum += all k-mer
 * occurrences of the window.  The receiver walks what it was sent with tsx_hip_shard_walk_device (long_desc = 2: every key
 * stays, the calls of a step -- slot 0 .. nslots - 1 -- append to ONE set of level-1 lists) and
 * builds with tsx_hip_shard_build_l1_device.  tsx_hip_mini_owner_host: the owner of each one-limb k-mer (lookups). */
int tsx_hip_mini_supported(tsx_hip_map *m);
int tsx_hip_mini_capacity(tsx_hip_map *m, size_t text_bytes, int nranks, size_t *descs_per_owner_out);
int tsx_hip_mini_window_device(tsx_hip_map *m, const void *dev_text, size_t n_total, size_t win_off, size_t win_len,
                               int nranks, void *dev_desc, size_t cap_per_owner, void *dev_counts, void *dev_kmer_sum,
                               void *stream);
/* The same in two steps, for a step of several exchange windows: the text is described ONCE (line pass + strip descriptions,
 * kept in the map's scratch until the next describe), then split share by share -- share `part` of `nparts` of the described
 * strips, lists and counts as above, cap_per_owner >= tsx_hip_mini_part_capacity(len, nparts) -- so that the exchange of one
 * share runs while the next is split and the one before is walked.  dev_kmer_sum += all k-mer occurrences of the text. */
int tsx_hip_mini_part_capacity(tsx_hip_map *m, size_t text_bytes, uint32_t nparts, size_t *descs_per_owner_out);
int tsx_hip_mini_describe_device(tsx_hip_map *m, const void *dev_text, size_t n_total, size_t off, size_t len, void *dev_kmer_sum,
                                 void *stream);
int tsx_hip_mini_split_device(tsx_hip_map *m, uint32_t part, uint32_t nparts, int nranks, void *dev_desc, size_t cap_per_owner,
                              void *dev_counts, void *stream);
int tsx_hip_mini_owner_host(int k, int nranks, const uint64_t *kmers, size_t n, uint32_t *owners_out);


/*
 * The multi-GPU run as ONE call from C++ (src/mains/main.cpp:404-507: one command runs the job): a group is one table per
 * GPU of this node, driven by one host thread per GPU inside the library (csrc/tsx_multi.cpp).
 *   group_create            ngpus tables (devices[r] = HIP ordinal of rank r, NULL = 0..ngpus-1).  comm 0 = RCCL
 *                           (ncclCommInitAll; librccl is loaded on demand; one GPU per rank), comm 1 = device-to-device
 *                           copies behind a barrier (ranks may share a GPU: tests of world sizes the box cannot give RCCL)
 *   group_count_fastq_host  countKMers for N GPUs: the text is cut into ngpus shards of whole records (empty lines
 *                           dropped, 4 or 2 lines per record: FastXReader.h:62-116,307-385), rank r counts shard r into
 *                           its own table (tsx_hip_count_fastq_host), then group_merge
 *   group_merge             the merge of the per-GPU tables: entries grouped by owner = tsx_hip_owner(kmer, ngpus)
 *                           (tsx_hip_partition_device), ONE all-to-all of k-mers and counts, the owner clears and
 *                           re-inserts (tsx_hip_add_kmers_device).  Afterwards every k-mer lives on the GPU that owns it
 *   group_get_counts_host   getKmerCount(kmer) (TSXHashMap.h:548-638): every k-mer is asked of its owner
 *   group_get_stats         sums over the GPUs (distinct = getKmerCount(), TSXHashMap.h:645)
 * tsx_hip_group_map gives the table of one rank for everything else in this header.
 */
typedef struct tsx_hip_group tsx_hip_group;
int tsx_hip_group_create(tsx_hip_group **out, int ngpus, const int *devices, int k, int l, int storagebits,
                         int overflow_l, uint64_t hash_seed, int comm);
void tsx_hip_group_destroy(tsx_hip_group *g);
int tsx_hip_group_size(const tsx_hip_group *g);
tsx_hip_map *tsx_hip_group_map(tsx_hip_group *g, int rank);
const char *tsx_hip_group_comm_name(const tsx_hip_group *g);   /* "rccl" or "copy" */
const char *tsx_hip_group_last_error(void);
int tsx_hip_group_set_record_lines(tsx_hip_group *g, int lines);
/* tsx_hip_set_canonical on every rank's table (an empty group only); lookups then route the canonical form of a
 * k-mer to its owner.  Refused together with the minimizer exchange (either order): TSX_HIP_EINVAL. */
int tsx_hip_group_set_canonical(tsx_hip_group *g, int on);
/* tsx_hip_set_base_rule on every rank's table (at any time).  Refused together with the minimizer exchange (either
 * order): TSX_HIP_EINVAL. */
int tsx_hip_group_set_base_rule(tsx_hip_group *g, int acgt_only, int min_qual_char);
/* exchange 0 (default): every GPU counts its shard into its own table, the tables are merged afterwards (any k);
 * exchange 1: the minimizer exchange (20 <= k <= 32, at most 16 GPUs) -- strip descriptions travel to the GPU that owns
 * their k-mers' minimizer BEFORE anything is built, nothing is merged (tsx_hip_group_merge is then a no-op), lookups go to
 * tsx_hip_mini_owner_host(kmer). */
int tsx_hip_group_set_exchange(tsx_hip_group *g, int mode);
int tsx_hip_group_exchange(const tsx_hip_group *g);
int tsx_hip_group_clear(tsx_hip_group *g);
int tsx_hip_group_count_fastq_host(tsx_hip_group *g, const char *text, size_t n);
int tsx_hip_group_merge(tsx_hip_group *g);
int tsx_hip_group_get_counts_host(tsx_hip_group *g, const uint64_t *kmers, size_t n, uint64_t *counts_out);
int tsx_hip_group_get_stats(tsx_hip_group *g, tsx_hip_stats *out);
uint64_t tsx_hip_group_exchanged_entries(const tsx_hip_group *g);   /* entries that changed GPU in the last merge */
/* Rounds of the last group_count_fastq_host (countKMers for N GPUs, main.cpp:104-218 + the exchange): pieces of the longest
 * shard x shares of a piece for the minimizer exchange, 0 for the merge.  A piece is 2 GiB of text and a share at least
 * 32 MiB; TSX_HIP_MZ_PIECE (bytes, rounded up to a multiple of 4096, 4096 .. 2 GiB) and TSX_HIP_MZ_SHARE (bytes, >= 1;
 * shares = piece / share, 1 .. 4) are read once per count and let tests put many rounds into a small text. */
uint32_t tsx_hip_group_exchange_rounds(const tsx_hip_group *g);
/* tsx_hip_histogram_host / tsx_hip_write_counts_host over the group, rank by rank: after group_count_fastq_host every
 * k-mer lives on one GPU (the merge leaves it on its owner; the minimizer exchange is disjoint by construction), so the
 * histogram is the sum of the ranks' and the file (the `.count` format of main.cpp:224-396) lists every k-mer once. */
int tsx_hip_group_histogram_host(tsx_hip_group *g, uint64_t *hist_out, size_t nbins);
int tsx_hip_group_write_counts_host(tsx_hip_group *g, int fd, uint64_t lower, uint64_t upper, size_t chunk_bytes,
                                    uint64_t *lines_out, uint64_t *bytes_out);
/* Where group_count_fastq_host cuts a text: cuts_out[0 .. parts], shard i = [cuts_out[i], cuts_out[i + 1]); every cut is
 * a record boundary of the reference's reader.  Host logic only (no GPU). */
int tsx_hip_cut_records_host(const char *text, size_t n, int parts, int lines_per_record, size_t *cuts_out);

/*
 * Synthetic reads shaped like generateFakeSequences.py (500-1000 random bases
 * + 100-300 'A', '@seq<i>' header, '&' qualities), written as FASTQ text
 * straight into device memory.  Sizing call: dev_out == NULL returns the byte
 * count in *bytes_out and the number of k-mers (for k) in *kmers_out.
 * tsxcount_amd/synth.py is the same generator on the host (numpy).
 */
int tsx_hip_synth_fastq_device(uint64_t seed, uint64_t first_read, uint64_t n_reads, int k,
                               void *dev_out, size_t cap, uint64_t *bytes_out, uint64_t *kmers_out,
                               uint64_t *polya_kmers_out, int device, void *stream);

/*
 * Zipf-skewed synthetic reads (BASELINE config 4: contention / reprobe stress): n_templates random template sequences of
 * 2 * read_len bases, read r = a window of read_len bases of template pick_r, pick_r Zipf distributed: thr (host,
 * n_templates ascending uint64) are the upper ends of the templates' shares of [0, 2^64).  '@z<r>' headers, 'I'
 * qualities.  Sizing call: dev_out == NULL.  tsxcount_amd/synth.py: zipf_thresholds(), the numpy twin and the analytic
 * count of every k-mer (what the bench's check compares the table with).
 */
int tsx_hip_synth_zipf_device(uint64_t seed, uint64_t n_reads, uint32_t read_len, uint32_t n_templates, const uint64_t *thr,
                              void *dev_out, size_t cap, uint64_t *bytes_out, int device, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TSXCOUNT_HIP_H */
