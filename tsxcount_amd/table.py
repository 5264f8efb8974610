"""TSXHashMapHIP: one table on one GPU, the host mirror of the reference's TSXHashMap surface over the C ABI."""
import ctypes

import numpy as np

from ._abi import (BIN_STATS_DTYPE, EINVAL, ERANGE, JOINT_MAX_CELLS, NORMALIZE_ROUND, PAIR_MODES, PREFILTER_BITS,
                   READ_MEDIAN_DTYPE, READ_STATS_DTYPE, SEQ_INTERVAL_DTYPE, SEQ_STATS_DTYPE, SKETCH_PRECISIONS, TRIM_SPAN_DTYPE,
                   BinIO, BinTotals, CombineStats, HetStats, Layout, NormalizeTotals, PairIO, PairTotals, PrefilterTotals,
                   SketchTotals, Stats, TrimTotals, TSXException, _check, _fds, _fetch_records, _p, _stream, _upper,
                   _write_counts, bin_rule, combine_rule, encode, filter_rule, het_pair_dtype, het_rule, lib, median_rule,
                   min_qual_code, normalize_rule, trim_rule)
from .textio import database_info

_vp = ctypes.c_void_p
_u8p = ctypes.POINTER(ctypes.c_uint8)


def _sketch_precision(registers):
    n = len(registers)
    p = n.bit_length() - 1
    if n != 1 << p or p not in SKETCH_PRECISIONS:
        raise ValueError("a sketch has 2^10 .. 2^14 registers, not %d" % n)
    return p


def sketch_estimate(registers):
    """The number of distinct k-mers a sketch stands for (tsx_hip_sketch_estimate_host): a float, 0.0 for an empty sketch."""
    r = np.ascontiguousarray(registers, dtype=np.uint8)
    e = lib().tsx_hip_sketch_estimate_host(r.ctypes.data_as(_u8p), _sketch_precision(r))
    if e < 0:
        raise TSXException(EINVAL, "a register above its highest rank")
    return float(e)


def suggest_l(distinct, k, load=0.75, precision=14):
    """The l (log2 of the slot count) of the smallest table that holds `distinct` k-mers at `load` with a margin of five
    standard errors of a sketch of 2^precision registers (tsx_hip_suggest_l): at least 4, at most min(36, 2k - 1).
    Where that bound leaves the load above 0.9: TSXException ERANGE, its .l the bound."""
    l = ctypes.c_int(0)
    rc = lib().tsx_hip_suggest_l(int(k), float(distinct), int(precision), int(round(float(load) * 1e6)), ctypes.byref(l))
    if rc == ERANGE:
        e = TSXException(rc, "l cannot exceed %d for k=%d: %.0f distinct k-mers load it above 0.9" % (l.value, k, distinct))
        e.l = int(l.value)
        raise e
    _check(rc)
    return int(l.value)


class TSXHashMapHIP:
    """Host mirror of TSXHashMap / TSXHashMapCAS for --mode=HIP.

    Constructor arguments follow TSXHashMap(iL, iStorageBits, iK)
    (TSXHashMap.h:79); method names follow the reference class.
    """

    def __init__(self, iL, iStorageBits, iK, iThreads=0, hash_seed=1, overflow_l=0, device=0, shard_bits=0,
                 shard_index=0, canonical=False, acgt_only=False, min_qual_char=None):
        min_qual_code(min_qual_char)   # (argument errors before anything is allocated)
        self._h = ctypes.c_void_p()
        self._lib = lib()
        _check(self._lib.tsx_hip_create_shard(ctypes.byref(self._h), iK, iL, iStorageBits, overflow_l,
                                              hash_seed, device, shard_bits, shard_index))
        self.layout = Layout()
        _check(self._lib.tsx_hip_get_layout(self._h, ctypes.byref(self.layout)))
        self.k, self.l, self.wk, self.device = iK, iL, self.layout.key_limbs, device
        self.hash_seed = hash_seed
        self.combine_stats = None
        self._lines = 4
        if canonical:
            self.set_canonical(True)
        if acgt_only or min_qual_char:
            self.set_base_rule(acgt_only, min_qual_char)

    @property
    def base_rule(self):
        """(acgt_only, min_qual_char) in effect: min_qual_char as a one-character str, None when off."""
        a, q = ctypes.c_int(), ctypes.c_int()
        _check(self._lib.tsx_hip_get_base_rule(self.handle, ctypes.byref(a), ctypes.byref(q)))
        return bool(a.value), (chr(q.value) if q.value else None)

    def set_base_rule(self, acgt_only=False, min_qual_char=None):
        """Which windows count as k-mers (tsx_hip_set_base_rule): acgt_only drops windows with a byte outside ACGTacgt,
        min_qual_char (a one-character str or an int) those with a base whose quality byte is below it or missing.
        Keys do not change, so the rule may change between calls; FASTQ only for min_qual_char."""
        q = min_qual_code(min_qual_char)
        if q and self._lines != 4:
            raise ValueError("min_qual_char needs FASTQ records: a FASTA text has no quality line")
        _check(self._lib.tsx_hip_set_base_rule(self.handle, 1 if acgt_only else 0, q))

    @property
    def canonical(self):
        """True when x and its reverse complement share one counter (tsx_hip_set_canonical)."""
        return self._lib.tsx_hip_canonical(self.handle) == 1

    def set_canonical(self, on=True):
        """Canonical counting on or off; an empty table only (just created or after clear())."""
        _check(self._lib.tsx_hip_set_canonical(self.handle, 1 if on else 0))

    def close(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            self._lib.tsx_hip_destroy(h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter teardown: ctypes may already be gone
            pass

    @property
    def handle(self):
        if self._h is None:
            raise TSXException(EINVAL, "map is closed")
        return self._h

    # --- reference surface -------------------------------------------------
    def getK(self):
        return self.k

    def getMaxElements(self):
        return int(self.layout.slots)

    def addKmer(self, kmer):
        """TSXHashMap::addKmer (TSXHashMap.h:182); kmer = limbs or sequence."""
        self.addKmers(self._as_kmers([kmer]))
        return True

    def addKmers(self, kmers, counts=None):
        a = np.ascontiguousarray(kmers, dtype=np.uint64).reshape(-1, self.wk)
        c = None
        if counts is not None:
            c = np.ascontiguousarray(counts, dtype=np.uint64)
            assert c.shape[0] == a.shape[0]
        _check(self._lib.tsx_hip_add_kmers_host(self._h, _p(a), _p(c) if c is not None else None, a.shape[0]))

    def getKmerCount(self, kmer=None):
        """getKmerCount(kmer) (TSXHashMap.h:548) or getKmerCount() (:645)."""
        if kmer is None:
            return self.stats()["distinct"]
        return int(self.getKmerCounts(self._as_kmers([kmer]))[0])

    def getKmerCounts(self, kmers):
        a = np.ascontiguousarray(kmers, dtype=np.uint64).reshape(-1, self.wk)
        out = np.zeros(a.shape[0], dtype=np.uint64)
        _check(self._lib.tsx_hip_get_counts_host(self._h, _p(a), a.shape[0], _p(out)))
        return out

    def getKmerCountDebug(self, kmers):
        """getKmerCountDebug (TSXHashMap.h:477): (counts, slots); slot = 2^64-1 for absent k-mers."""
        a = np.ascontiguousarray(kmers, dtype=np.uint64).reshape(-1, self.wk)
        out = np.zeros(a.shape[0], dtype=np.uint64)
        pos = np.zeros(a.shape[0], dtype=np.uint64)
        _check(self._lib.tsx_hip_lookup_host(self._h, _p(a), a.shape[0], _p(out), _p(pos)))
        return out, pos

    def getKmerStarts(self):
        """getKmerStarts (TSXHashMap.h:650) as a numpy bool array over the 2^l slots."""
        nb = (int(self.layout.slots) + 7) // 8
        bits = np.zeros(nb, dtype=np.uint8)
        _check(self._lib.tsx_hip_kmer_starts_host(self._h, bits.ctypes.data_as(_u8p), nb))
        return np.unpackbits(bits, bitorder="little")[:int(self.layout.slots)].astype(bool)

    def getAllKmers(self):
        """TSXHashMap::getAllKmers (TSXHashMap.h:660) with counts; order unspecified."""
        n = self.stats()["distinct"]
        kmers = np.zeros((max(n, 1), self.wk), dtype=np.uint64)
        counts = np.zeros(max(n, 1), dtype=np.uint64)
        got = ctypes.c_size_t(0)
        _check(self._lib.tsx_hip_dump_host(self._h, _p(kmers), _p(counts), max(n, 1), ctypes.byref(got)))
        return kmers[:got.value], counts[:got.value]

    def dumpRangeDevice(self, slot_lo, slot_hi, kmers_ptr, counts_ptr, cap, n_ptr, stream=None):
        """getAllKmers for the slots [slot_lo, slot_hi) into device buffers (tsx_hip_dump_range_device)."""
        _check(self._lib.tsx_hip_dump_range_device(self._h, slot_lo, slot_hi, _vp(kmers_ptr), _vp(counts_ptr), cap,
                                                   _vp(n_ptr), _stream(stream)))

    def getCountHistogram(self, nbins=10002, slot_lo=0, slot_hi=None):
        """Abundance histogram (numpy uint64, nbins): [c] = k-mers counted c times, the last bin pools every count
        >= nbins - 1.  The whole table, or the slots [slot_lo, slot_hi) (tsx_hip_histogram_device on a torch buffer)."""
        out = np.zeros(nbins, dtype=np.uint64)
        if slot_lo == 0 and slot_hi is None:
            _check(self._lib.tsx_hip_histogram_host(self._h, _p(out), nbins))
            return out
        import torch
        hi = int(self.layout.slots) if slot_hi is None else int(slot_hi)
        buf = torch.empty(max(nbins, 1), dtype=torch.int64, device=torch.device("cuda", self.device))
        st = torch.cuda.Stream(buf.device)   # a stream of its own: torch's default one does not wait for the map's
        _check(self._lib.tsx_hip_histogram_device(self._h, int(slot_lo), hi, nbins, _vp(buf.data_ptr()), _vp(st.cuda_stream)))
        st.synchronize()
        out[:] = buf.cpu().numpy().view(np.uint64)
        return out

    def writeCounts(self, path, lower=1, upper=None, chunk_bytes=0):
        """Every k-mer whose count lies in [lower, upper] as "kmer<TAB>count" lines (the .count format of
        count_kmers.py / main.cpp:224-396) to a path (created or truncated) or an open file descriptor, in no
        particular order.  Returns (lines, bytes)."""
        return _write_counts(self._lib.tsx_hip_write_counts_host, self.handle, _check, path, lower, upper, chunk_bytes)

    def saveDatabase(self, path_or_fd, chunk_bytes=0):
        """The table as a k-mer database (tsx_hip_save_host) to a path (created or truncated) or an open file descriptor
        (written from its current position).  Returns (entries, bytes written)."""
        entries, nbytes = ctypes.c_uint64(0), ctypes.c_uint64(0)
        with _fds(path_or_fd) as (fd,):
            rc = self._lib.tsx_hip_save_host(self.handle, fd, int(chunk_bytes), ctypes.byref(entries), ctypes.byref(nbytes))
        _check(rc)
        return int(entries.value), int(nbytes.value)

    def addDatabase(self, path_or_fd, chunk_bytes=0):
        """Load a k-mer database into this table (tsx_hip_load_host): placed as it is into an empty table of the same
        geometry and seed, otherwise every k-mer is added with its count (a merge).  Returns the entries read.  After an
        error the table's content is unspecified: clear() recovers it."""
        entries = ctypes.c_uint64(0)
        with _fds(path_or_fd, read=True) as (fd,):
            rc = self._lib.tsx_hip_load_host(self.handle, fd, int(chunk_bytes), ctypes.byref(entries))
        _check(rc)
        return int(entries.value)

    @classmethod
    def fromDatabase(cls, path, iL=None, iStorageBits=None, device=0, chunk_bytes=0):
        """A new table holding a k-mer database: k, seed, counting mode and base rule come from the file; l and the
        storage bits too unless given (a different geometry loads through the re-insert path)."""
        info = database_info(path)
        same = iL in (None, info["l"]) and iStorageBits in (None, info["count_bits"])
        m = cls(info["l"] if iL is None else iL, info["count_bits"] if iStorageBits is None else iStorageBits, info["k"],
                hash_seed=info["hash_seed"], overflow_l=info["overflow_l"] if same else 0, device=device,
                canonical=bool(info["canonical"]), acgt_only=bool(info["acgt_only"]), min_qual_char=info["min_qual_char"] or None)
        try:
            m.addDatabase(path, chunk_bytes)
        except Exception:
            m.close()
            raise
        return m

    # --- two tables: set operations, joint spectrum, read binning ------------------------------------------------------
    def _combine(self, other, rule, out):
        st = CombineStats()
        _check(self._lib.tsx_hip_combine(out.handle if out is not None else None, self.handle, other.handle,
                                         ctypes.byref(rule), ctypes.byref(st)), refusal=True)
        return st.as_dict()

    def combine(self, other, op="intersect", counts="min", a_range=(1, None), b_range=(1, None), out=None, iL=None,
                iStorageBits=None, hash_seed=None):
        """Set operation on two tables (tsx_hip_combine): self is A, `other` is B.  op: "intersect", "union",
        "subtract" (A's k-mers that B lacks) or "diff" (count differences a - b > 0); counts: "min", "max", "sum",
        "left", "right" where a k-mer is in both; a_range / b_range: (lower, upper) of the counts that take part.
        Returns the result table with .combine_stats set: `out` (an empty map) when given, else a new map created like
        self -- same l, storage bits and seed unless iL / iStorageBits / hash_seed say otherwise."""
        rule = combine_rule(op, counts, a_range, b_range)
        made = out is None
        if made:
            same = iL in (None, self.l) and iStorageBits in (None, self.layout.count_bits)
            acgt, minq = self.base_rule
            out = TSXHashMapHIP(self.l if iL is None else iL,
                                self.layout.count_bits if iStorageBits is None else iStorageBits, self.k,
                                hash_seed=self.hash_seed if hash_seed is None else hash_seed,
                                overflow_l=self.layout.overflow_l if same else 0, device=self.device,
                                canonical=self.canonical, acgt_only=acgt, min_qual_char=minq)
        try:
            out.combine_stats = self._combine(other, rule, out)
        except Exception:
            if made:
                out.close()
            raise
        return out

    def compare(self, other, a_range=(1, None), b_range=(1, None)):
        """How two tables overlap (tsx_hip_combine without an output table): the combine stats of an intersection
        -- a_in_range, b_in_range, both, a_sum_both, b_sum_both, ... -- plus `jaccard` = both / (a + b - both)."""
        st = self._combine(other, combine_rule("intersect", "min", a_range, b_range), None)
        union = st["a_in_range"] + st["b_in_range"] - st["both"]
        st["jaccard"] = st["both"] / union if union else 0.0
        return st

    def jointHistogram(self, other, bins_a=1002, bins_b=1002):
        """Joint k-mer spectrum of two tables (tsx_hip_joint_histogram_host; KAT `comp`): self is A, `other` is B.
        Returns numpy uint64[bins_a, bins_b]: [i, j] = distinct k-mers counted i times in A and j times in B, the last
        bin of each side pooling every larger count; [0, 0] is 0.  joint_histogram() states the definition."""
        out = np.zeros((int(bins_a), int(bins_b)) if 0 < bins_a * bins_b <= JOINT_MAX_CELLS else (0, 0), dtype=np.uint64)
        _check(self._lib.tsx_hip_joint_histogram_host(self.handle, other.handle, _p(out), int(bins_a), int(bins_b)), refusal=True)
        return out

    def jointHistogramDevice(self, other, matrix_ptr, bins_a=1002, bins_b=1002, stream=None):
        """tsx_hip_joint_histogram_device: the matrix into uint64[bins_a * bins_b] in device memory (zeroed by the call),
        queued on `stream` (None = this map's own); returns without waiting."""
        _check(self._lib.tsx_hip_joint_histogram_device(self.handle, other.handle, int(bins_a), int(bins_b), _vp(matrix_ptr),
                                                        _stream(stream)), refusal=True)

    def binStats(self, other, text, a_range=(1, None), b_range=(1, None), min_hits=1, ratio=1.0, chunk_bytes=0):
        """Hits of every record of a FASTQ / FASTA text in two tables, in one scan (tsx_hip_bin_stats_host): self is A,
        `other` is B.  Returns (stats, classes): a numpy structured array (BIN_STATS_DTYPE: kmers, hits_a, hits_b,
        hits_both) and a uint8 array of BIN_A / BIN_B / BIN_AMBIGUOUS / BIN_NONE, one entry per record in text order.
        A window hits a table when its count there lies in the table's range; bin_class() states the class rule."""
        b = bytes(text)
        rule = bin_rule(a_range, b_range, min_hits, ratio)
        classes = [None]   # (as long as the stats of the attempt that went through)

        def call(out, cap, n):
            classes[0] = np.zeros(cap, dtype=np.uint8)
            return self._lib.tsx_hip_bin_stats_host(self.handle, other.handle, b, len(b), ctypes.byref(rule), out,
                                                    classes[0].ctypes.data_as(_vp), cap, n, int(chunk_bytes))
        stats = _fetch_records(BIN_STATS_DTYPE, len(b), call, refusal=True)
        return stats, classes[0][:len(stats)]

    def binStatsDevice(self, other, text_ptr, nbytes, stats_ptr, cap, a_range=(1, None), b_range=(1, None), min_hits=1,
                       ratio=1.0, stream=None):
        """tsx_hip_bin_stats_device: the bin stats of the records of a device text into a device buffer of cap records
        (4 uint64 each).  Waits; returns the record count (more than cap: TSXException ERANGE)."""
        rule = bin_rule(a_range, b_range, min_hits, ratio)
        n = ctypes.c_size_t(0)
        _check(self._lib.tsx_hip_bin_stats_device(self.handle, other.handle, _vp(text_ptr), nbytes, ctypes.byref(rule),
                                                  _vp(stats_ptr), cap, ctypes.byref(n), _stream(stream)), refusal=True)
        return int(n.value)

    def binReads(self, other, text, out_a=None, out_b=None, out_ambiguous=None, out_none=None, a_range=(1, None),
                 b_range=(1, None), min_hits=1, ratio=1.0, chunk_bytes=0):
        """Split the records of `text` by the table they hit more (tsx_hip_bin_reads_host): self is A, `other` is B.
        Each output is a path (created or truncated), an open file descriptor, or None (the class is counted and not
        written); at least one is needed.  Returns the totals as a dict: records, n[class], bytes[class]."""
        b = bytes(text)
        rule = bin_rule(a_range, b_range, min_hits, ratio)
        with _fds(out_a, out_b, out_ambiguous, out_none) as fds:
            io, tot = BinIO(*fds), BinTotals()
            rc = self._lib.tsx_hip_bin_reads_host(self.handle, other.handle, b, len(b), ctypes.byref(rule), ctypes.byref(io),
                                                  int(chunk_bytes), ctypes.byref(tot))
        _check(rc, refusal=True)
        return tot.as_dict()

    # --- heterozygous k-mer pairs ----------------------------------------------------------------------------------------
    def hetHistogram(self, bins_minor=1002, bins_major=1002, lower=1, upper=None, mode="unique"):
        """Heterozygous k-mer pairs of this table by their two counts (tsx_hip_het_histogram_host; Smudgeplot's hetkmers):
        the pairs of k-mers counted in [lower, upper] that differ only in their middle base.  mode 'unique' counts the pair
        of a family of exactly two, 'all' every pair of every family.  Returns (numpy uint64[bins_minor, bins_major], stats):
        [i, j] = pairs whose lower count is i and whose higher count is j, the last bin of each side pooling every larger
        count; stats is the dict of het_pairs().  het_pairs() and het_histogram() state the definition.  k must be odd."""
        rule = het_rule(lower, upper, mode)
        ok = bins_minor > 0 and bins_major > 0 and bins_minor * bins_major <= JOINT_MAX_CELLS
        out = np.zeros((int(bins_minor), int(bins_major)) if ok else (0, 0), dtype=np.uint64)
        st = HetStats()
        _check(self._lib.tsx_hip_het_histogram_host(self.handle, ctypes.byref(rule), _p(out), int(bins_minor), int(bins_major),
                                                    ctypes.byref(st)), refusal=True)
        return out, {n: int(getattr(st, n)) for n, _ in HetStats._fields_}

    def hetHistogramDevice(self, matrix_ptr, stats_ptr, bins_minor=1002, bins_major=1002, lower=1, upper=None, mode="unique",
                           stream=None):
        """tsx_hip_het_histogram_device: the matrix into uint64[bins_minor * bins_major] and the five totals into uint64[5],
        both in device memory (zeroed by the call), queued on `stream` (None = this map's own); returns without waiting."""
        rule = het_rule(lower, upper, mode)
        _check(self._lib.tsx_hip_het_histogram_device(self.handle, ctypes.byref(rule), int(bins_minor), int(bins_major),
                                                      _vp(matrix_ptr), _vp(stats_ptr), _stream(stream)), refusal=True)

    def hetPairs(self, lower=1, upper=None, mode="unique", slot_lo=0, slot_hi=None, range_slots=1 << 20):
        """The heterozygous pairs themselves (tsx_hip_het_pairs_device, range_slots slots a call): a numpy structured
        array het_pair_dtype(k) -- minor, major (k-mers as limbs, as a dump reports them), minor_count, major_count -- in
        no particular order.  The record's width follows the key width, so the dtype is het_pair_dtype(self.k); it equals
        HET_PAIR_DTYPE only for one-limb keys (k <= 32).  slot_lo / slot_hi: only the pairs those slots own (every pair is owned by one slot)."""
        import torch
        rule = het_rule(lower, upper, mode)
        dt = het_pair_dtype(self.k)
        hi = int(self.layout.slots) if slot_hi is None else int(slot_hi)
        step = max(1, int(range_slots))
        cap = min(step, max(hi - int(slot_lo), 1)) * (3 if mode == "all" else 1)
        words = dt.itemsize // 8
        buf = torch.empty(cap * words + 1, dtype=torch.int64, device=torch.device("cuda", self.device))
        st = torch.cuda.Stream(buf.device)   # a stream of its own: torch's default one does not wait for the map's
        parts = []
        lo = int(slot_lo)
        while True:
            top = min(hi, lo + step)
            _check(self._lib.tsx_hip_het_pairs_device(self.handle, ctypes.byref(rule), lo, top, _vp(buf.data_ptr()), cap,
                                                      _vp(buf.data_ptr() + cap * words * 8), _vp(st.cuda_stream)), refusal=True)
            n = int(buf[cap * words].item())
            if n:
                parts.append(buf[:n * words].cpu().numpy().view(np.uint64).view(dt).copy())
            lo = top
            if lo >= hi:
                break
        return np.concatenate(parts) if parts else np.zeros(0, dtype=dt)

    def writeHetPairs(self, path_or_fd, lower=1, upper=None, mode="unique", chunk_bytes=0):
        """The pairs as "minor_kmer<TAB>minor_count<TAB>major_kmer<TAB>major_count" lines (tsx_hip_write_het_pairs_host) to
        a path (created or truncated) or an open file descriptor, in no particular order.  Returns (pairs, bytes)."""
        rule = het_rule(lower, upper, mode)
        pairs, nbytes = ctypes.c_uint64(0), ctypes.c_uint64(0)
        with _fds(path_or_fd) as (fd,):
            rc = self._lib.tsx_hip_write_het_pairs_host(self.handle, ctypes.byref(rule), fd, int(chunk_bytes), ctypes.byref(pairs),
                                                        ctypes.byref(nbytes))
        _check(rc, refusal=True)
        return int(pairs.value), int(nbytes.value)

    # --- read queries ------------------------------------------------------------------------------------------------------
    def queryReads(self, text, lower=1, upper=None, chunk_bytes=0):
        """Per-record k-mer stats of a FASTQ / FASTA text against the table (tsx_hip_query_reads_host): a numpy
        structured array (READ_STATS_DTYPE: kmers, in_range, min_count, sum_count), one entry per record in text
        order; in_range counts the k-mers whose count lies in [lower, upper]."""
        b = bytes(text)
        return _fetch_records(READ_STATS_DTYPE, len(b), lambda out, cap, n: self._lib.tsx_hip_query_reads_host(
            self.handle, b, len(b), int(lower), _upper(upper), out, cap, n, int(chunk_bytes)))

    # --- sequence queries: the sequences of a wrapped FASTA (csrc/tsx_seq.h) ---------------------------------------
    def _seq_call(self, fn, args, use):
        """Runs one tsx_hip_seq_* entry point and hands its result to use(res) before it is freed."""
        res = ctypes.c_void_p(None)
        _check(fn(self.handle, *args, ctypes.byref(res)), refusal=True)
        try:
            return use(res)
        finally:
            self._lib.tsx_hip_seq_result_free(res)

    def _seq_stats_of(self, res):
        L = self._lib
        n = L.tsx_hip_seq_result_count(res)
        stats = np.zeros(n, dtype=SEQ_STATS_DTYPE)
        if n:
            ctypes.memmove(stats.ctypes.data, L.tsx_hip_seq_result_stats(res), n * SEQ_STATS_DTYPE.itemsize)
        offs = ctypes.c_void_p(None)
        blob = L.tsx_hip_seq_result_names(res, ctypes.byref(offs))
        off = np.zeros(n + 1, dtype=np.uint64)
        ctypes.memmove(off.ctypes.data, offs.value, (n + 1) * 8)
        raw = ctypes.string_at(blob, int(off[n])) if int(off[n]) else b""
        return [raw[int(off[i]):int(off[i + 1])] for i in range(n)], stats

    def _seq_intervals_of(self, res):
        iv = ctypes.c_void_p(None)
        n = self._lib.tsx_hip_seq_result_intervals(res, ctypes.byref(iv))
        out = np.zeros(n, dtype=SEQ_INTERVAL_DTYPE)
        if n:
            ctypes.memmove(out.ctypes.data, iv.value, n * SEQ_INTERVAL_DTYPE.itemsize)
        return out

    def querySequences(self, text, lower=1, upper=None, chunk_bytes=0):
        """Per-sequence k-mer stats of a wrapped FASTA text against the table (tsx_hip_seq_stats_host): (names, stats)
        -- a list of bytes and a numpy structured array (SEQ_STATS_DTYPE), one entry per record of fasta_records(text);
        what sequence_stats states on the CPU."""
        b = bytes(text)
        return self._seq_call(self._lib.tsx_hip_seq_stats_host, (b, len(b), int(lower), _upper(upper), int(chunk_bytes)),
                              self._seq_stats_of)

    def missingIntervals(self, text, lower=1, upper=None, chunk_bytes=0):
        """The maximal runs of missing k-mers of every sequence (tsx_hip_seq_missing_host): a numpy structured array
        (SEQ_INTERVAL_DTYPE: seq, start, end), ordered by sequence, then start; what missing_intervals states."""
        b = bytes(text)
        return self._seq_call(self._lib.tsx_hip_seq_missing_host, (b, len(b), int(lower), _upper(upper), int(chunk_bytes)),
                              self._seq_intervals_of)

    def querySequencesBgzf(self, gz, lower=1, upper=None):
        """querySequences for the image of a blocked gzip (BGZF) file."""
        b = bytes(gz)
        return self._seq_call(self._lib.tsx_hip_seq_stats_bgzf_host, (b, len(b), int(lower), _upper(upper)), self._seq_stats_of)

    def missingIntervalsBgzf(self, gz, lower=1, upper=None):
        """missingIntervals for the image of a blocked gzip (BGZF) file."""
        b = bytes(gz)
        return self._seq_call(self._lib.tsx_hip_seq_missing_bgzf_host, (b, len(b), int(lower), _upper(upper)),
                              self._seq_intervals_of)

    def querySequencesDevice(self, text_ptr, nbytes, lower=1, upper=None, missing=False, stream=None):
        """querySequences for a wrapped FASTA text resident on the device (16-byte aligned): (names, stats), and the
        intervals as a third item when missing is set (tsx_hip_seq_stats_device / tsx_hip_seq_missing_device)."""
        fn = self._lib.tsx_hip_seq_missing_device if missing else self._lib.tsx_hip_seq_stats_device

        def call(handle, *a):
            return fn(handle, *a, _stream(stream))
        use = (lambda r: self._seq_stats_of(r) + (self._seq_intervals_of(r),)) if missing else self._seq_stats_of
        return self._seq_call(call, (_vp(text_ptr), nbytes, int(lower), _upper(upper)), use)

    def _seq_write(self, text, path_or_fd, lower, upper, chunk_bytes, missing):
        b = bytes(text)
        fn = self._lib.tsx_hip_seq_missing_host if missing else self._lib.tsx_hip_seq_stats_host
        with _fds(path_or_fd) as (fd,):
            def use(res):
                if missing:
                    _check(self._lib.tsx_hip_seq_write_missing(res, fd))
                    return len(self._seq_intervals_of(res))
                _check(self._lib.tsx_hip_seq_write_stats(res, self.k, fd))
                return int(self._lib.tsx_hip_seq_result_count(res))
            return self._seq_call(fn, (b, len(b), int(lower), _upper(upper), int(chunk_bytes)), use)

    def writeSequenceStats(self, text, path_or_fd, lower=1, upper=None, chunk_bytes=0):
        """One line per sequence to a path or an open file descriptor: name, length, kmers, present, missing, min, sum,
        qv (tsx_hip_seq_write_stats).  Returns the number of sequences."""
        return self._seq_write(text, path_or_fd, lower, upper, chunk_bytes, False)

    def writeMissing(self, text, path_or_fd, lower=1, upper=None, chunk_bytes=0):
        """The missing intervals as BED (name, start, end) to a path or an open file descriptor.  Returns their number."""
        return self._seq_write(text, path_or_fd, lower, upper, chunk_bytes, True)

    # --- read filter, trim, medians ----------------------------------------------------------------------------------------
    def filterReads(self, text, path_or_fd, lower=2, upper=None, min_in_range=0, fraction=1.0, invert=False, chunk_bytes=0):
        """Write the records of `text` whose k-mers pass the rule (tsx_hip_filter_reads_host) to a path (created or
        truncated) or an open file descriptor.  Returns (records kept, bytes written)."""
        b = bytes(text)
        rule = filter_rule(lower, upper, min_in_range, fraction, invert)
        kept, nbytes = ctypes.c_uint64(0), ctypes.c_uint64(0)
        with _fds(path_or_fd) as (fd,):
            rc = self._lib.tsx_hip_filter_reads_host(self.handle, b, len(b), ctypes.byref(rule), fd, int(chunk_bytes),
                                                     ctypes.byref(kept), ctypes.byref(nbytes))
        _check(rc)
        return int(kept.value), int(nbytes.value)

    def trimSpans(self, text, lower=2, upper=None, mode="longest", chunk_bytes=0):
        """The kept span of every record of a FASTQ / FASTA text (tsx_hip_trim_spans_host): a numpy structured array
        (TRIM_SPAN_DTYPE: start, length in bases of the sequence line), one entry per record in text order.  A window
        is solid when its count lies in [lower, upper]; mode "longest" keeps the longest run of solid windows (the
        leftmost among equals), "prefix" the run that starts the read."""
        rule = trim_rule(lower, upper, mode)
        b = bytes(text)
        return _fetch_records(TRIM_SPAN_DTYPE, len(b), lambda out, cap, n: self._lib.tsx_hip_trim_spans_host(
            self.handle, b, len(b), ctypes.byref(rule), out, cap, n, int(chunk_bytes)))

    def trimReads(self, text, path_or_fd, lower=2, upper=None, mode="longest", min_len=0, chunk_bytes=0):
        """Write the records of `text` cut to their kept spans (tsx_hip_trim_reads_host) to a path (created or
        truncated) or an open file descriptor; records that keep fewer than min_len bases (0 = k) are dropped.  Returns
        the totals as a dict: records, kept, bases_in, bases_kept, bytes."""
        rule = trim_rule(lower, upper, mode, min_len)
        b = bytes(text)
        tot = TrimTotals()
        with _fds(path_or_fd) as (fd,):
            rc = self._lib.tsx_hip_trim_reads_host(self.handle, b, len(b), ctypes.byref(rule), fd, int(chunk_bytes),
                                                   ctypes.byref(tot))
        _check(rc)
        return tot.as_dict()

    def countProfile(self, text, chunk_bytes=0):
        """The count of every window of a FASTQ / FASTA text (tsx_hip_count_profile_host): numpy uint32[len(text)],
        entry i = min(count, 0xFFFFFFFE) of the k-mer that starts at byte i, NO_KMER where none does."""
        b = bytes(text)
        out = np.empty(len(b), dtype=np.uint32)
        _check(self._lib.tsx_hip_count_profile_host(self.handle, b, len(b), out.ctypes.data_as(_vp), int(chunk_bytes)))
        return out

    def medianReads(self, text, chunk_bytes=0):
        """The median k-mer count of every record of a FASTQ / FASTA text (tsx_hip_median_reads_host): a numpy
        structured array (READ_MEDIAN_DTYPE: kmers, median), one entry per record in text order; the median is that of
        median_count over the record's profile entries."""
        b = bytes(text)
        return _fetch_records(READ_MEDIAN_DTYPE, len(b), lambda out, cap, n: self._lib.tsx_hip_median_reads_host(
            self.handle, b, len(b), out, cap, n, int(chunk_bytes)))

    def filterReadsByMedian(self, text, path_or_fd, lower=0, upper=None, invert=False, chunk_bytes=0):
        """Write the records of `text` whose median k-mer count lies in [lower, upper] (tsx_hip_filter_median_host) to
        a path (created or truncated) or an open file descriptor; invert writes the others.  Returns (records kept,
        bytes written)."""
        rule = median_rule(lower, upper, invert)
        b = bytes(text)
        kept, nbytes = ctypes.c_uint64(0), ctypes.c_uint64(0)
        with _fds(path_or_fd) as (fd,):
            rc = self._lib.tsx_hip_filter_median_host(self.handle, b, len(b), ctypes.byref(rule), fd, int(chunk_bytes),
                                                      ctypes.byref(kept), ctypes.byref(nbytes))
        _check(rc)
        return int(kept.value), int(nbytes.value)

    def countProfileDevice(self, text_ptr, nbytes, profile_ptr, stream=None):
        """tsx_hip_count_profile_device: the profile of a device text into a device buffer of nbytes uint32."""
        _check(self._lib.tsx_hip_count_profile_device(self.handle, _vp(text_ptr), nbytes, _vp(profile_ptr), _stream(stream)))

    def medianReadsDevice(self, text_ptr, nbytes, medians_ptr, cap, stream=None):
        """tsx_hip_median_reads_device: {kmers, median} of the records of a device text into a device buffer of cap
        entries.  Returns the record count (more than cap: TSXException ERANGE)."""
        n = ctypes.c_size_t(0)
        _check(self._lib.tsx_hip_median_reads_device(self.handle, _vp(text_ptr), nbytes, _vp(medians_ptr), cap, ctypes.byref(n),
                                                     _stream(stream)))
        return int(n.value)

    # --- digital normalization ----------------------------------------------
    def normalizeReads(self, text, path_or_fd=None, cutoff=20, round_records=NORMALIZE_ROUND, keep=False, chunk_bytes=0):
        """Digital normalization (tsx_hip_normalize_host): the records of `text` in rounds of round_records; a record is
        kept iff the median count of its k-mers, in the table as it stands when its round starts, is below cutoff, and
        the k-mers of a round's kept records are counted when the round has been judged.  The kept records go to a
        path (created or truncated) or an open file descriptor; None: no output.  Returns the totals (records, kept,
        kmers_seen, kmers_added, rounds) as a dict; keep=True adds `keep`, a numpy bool array with one entry per
        record."""
        rule = normalize_rule(cutoff, round_records)
        b = bytes(text)
        tot = NormalizeTotals()
        flags = np.zeros(len(b) // 2 + 2 if keep else 0, dtype=np.uint8)   # (a record holds two bytes at least)
        with _fds(path_or_fd) as (fd,):
            rc = self._lib.tsx_hip_normalize_host(self.handle, b, len(b), ctypes.byref(rule), fd,
                                                  flags.ctypes.data_as(_vp) if keep else None, flags.size,
                                                  int(chunk_bytes), ctypes.byref(tot))
        _check(rc, refusal=True)
        out = tot.as_dict()
        if keep:
            out["keep"] = flags[:out["records"]].astype(bool)
        return out

    def normalizeReadsDevice(self, text_ptr, nbytes, keep_ptr, keep_cap, cutoff=20, round_records=NORMALIZE_ROUND, stream=None):
        """tsx_hip_normalize_device: the same for a device text; one byte per record into a device buffer of keep_cap
        bytes (keep_ptr None: no flags).  Returns the totals as a dict (more records than keep_cap: TSXException
        ERANGE, the table is complete)."""
        rule = normalize_rule(cutoff, round_records)
        tot = NormalizeTotals()
        _check(self._lib.tsx_hip_normalize_device(self.handle, _vp(text_ptr), nbytes, ctypes.byref(rule),
                                                  _vp(keep_ptr) if keep_ptr else None, keep_cap, ctypes.byref(tot),
                                                  _stream(stream)), refusal=True)
        return tot.as_dict()

    # --- table sizing -------------------------------------------------------
    def _sketch_regs(self, precision, registers):
        if int(precision) not in SKETCH_PRECISIONS:
            raise ValueError("sketch precision must be 10 .. 14, not %r" % (precision,))
        if registers is None:
            return np.zeros(1 << int(precision), dtype=np.uint8)
        r = np.array(registers, dtype=np.uint8)
        if r.shape != (1 << int(precision),):
            raise ValueError("registers: %d entries for precision %d" % (r.size, precision))
        return r

    def sketchKmers(self, text, precision=14, registers=None, chunk_bytes=0):
        """The HyperLogLog sketch of the k-mers `text` would put into this map (tsx_hip_sketch_host): (registers, totals)
        with registers numpy uint8[2^precision] -- those of sketch_registers over the k-mers the counting calls would
        count -- and totals {kmers: their exact number, records}.  registers= accumulates into a copy of an existing
        sketch.  The map gives k, the record lines, canonical and the base rule; its table is neither read nor written."""
        r = self._sketch_regs(precision, registers)
        b = bytes(text)
        t = SketchTotals()
        _check(self._lib.tsx_hip_sketch_host(self.handle, b, len(b), int(precision), r.ctypes.data_as(_u8p), ctypes.byref(t),
                                             int(chunk_bytes)))
        return r, t.as_dict()

    def sketchKmersBgzf(self, gz, precision=14, registers=None):
        """The same for the image of a blocked gzip (BGZF) file, inflated on the device (tsx_hip_sketch_bgzf_host)."""
        r = self._sketch_regs(precision, registers)
        b = bytes(gz)
        t = SketchTotals()
        _check(self._lib.tsx_hip_sketch_bgzf_host(self.handle, b, len(b), int(precision), r.ctypes.data_as(_u8p),
                                                  ctypes.byref(t)), refusal=True)
        return r, t.as_dict()

    def sketchKmersDevice(self, text_ptr, nbytes, regs_ptr, precision=14, totals_ptr=None, stream=None):
        """tsx_hip_sketch_device: the sketch of a device text max-combined into uint32[2^precision] in device memory;
        totals_ptr: two uint64 {kmers, records} in device memory, added to.  Queued, not waited for."""
        _check(self._lib.tsx_hip_sketch_device(self.handle, _vp(text_ptr), nbytes, int(precision), _vp(regs_ptr),
                                               _vp(totals_ptr) if totals_ptr else None, _stream(stream)))

    @classmethod
    def _smallest(cls, iK, iStorageBits, **kw):
        """A map of the smallest l that has a layout for iK and iStorageBits: 4, but a long k-mer needs its func bits to
        fit four limbs (k = 127: l >= 11)."""
        hi = min(36, 2 * iK - 1)
        for l in range(min(4, hi), hi + 1):
            try:
                return cls(l, iStorageBits, iK, **kw)
            except TSXException as e:
                if e.code != EINVAL or l == hi:
                    raise

    @classmethod
    def sizedFor(cls, text, iK, iStorageBits=0, load=0.75, precision=14, canonical=False, acgt_only=False, min_qual_char=None,
                 lines=4, **kw):
        """A map sized for `text`: the text is sketched on a minimal probe map that carries the counting mode, and the
        map returned has the l that suggest_l gives for the estimate (at least the smallest l that has a layout for iK:
        above 4 for k > 121 only).  Its .size_estimate is {kmers, distinct, l, load}
        (load: the expected one, distinct / 2^l).  Nothing is counted."""
        if lines not in (2, 4):
            raise ValueError("lines: 4 (FASTQ) or 2 (FASTA, one sequence line per record); wrapped FASTA has no sketch")
        dev = {n: kw[n] for n in ("device", "hash_seed") if n in kw}
        probe = cls._smallest(iK, iStorageBits, canonical=canonical, acgt_only=acgt_only, min_qual_char=min_qual_char, **dev)
        l_min = probe.l
        try:
            if lines != 4:
                probe.set_record_lines(lines)
            regs, tot = probe.sketchKmers(text, precision=precision)
        finally:
            probe.close()
        distinct = sketch_estimate(regs)
        l = max(l_min, suggest_l(distinct, iK, load=load, precision=precision))
        m = cls(l, iStorageBits, iK, canonical=canonical, acgt_only=acgt_only, min_qual_char=min_qual_char, **kw)
        if lines != 4:
            m.set_record_lines(lines)
        m.size_estimate = {"kmers": tot["kmers"], "distinct": distinct, "l": l, "load": distinct / float(1 << l)}
        return m

    # --- counting only the k-mers seen twice ----------------------------------
    def _prefilter_for(self, bits):
        """A filter for pass 1: the map's, when it has one and bits is None; else a new one of `bits` (None: l + 6, so that
        filter A takes the bytes of a one-limb table of 2^l slots; clamped to 12 .. 38)."""
        if bits is None:
            if self.prefilter_bits:
                return
            bits = min(max(self.l + 6, PREFILTER_BITS[0]), PREFILTER_BITS[-1])
        self.createPrefilter(bits)

    def createPrefilter(self, bits):
        """A new, empty prefilter of 2^bits bits (tsx_hip_prefilter_create; 12 .. 38), disarmed; replaces the one the map has."""
        _check(self._lib.tsx_hip_prefilter_create(self.handle, int(bits)))

    def freePrefilter(self):
        _check(self._lib.tsx_hip_prefilter_free(self.handle))

    def prefilter(self, text, bits=None, chunk_bytes=0):
        """Pass 1 of a count that keeps out the k-mers seen once (tsx_hip_prefilter_add_host): the k-mers of `text` -- those
        the counting calls would count -- into the map's prefilter.  bits: a new filter of that size first; None: the
        filter the map has (several texts accumulate), a new one of l + 6 bits when it has none.  Then armPrefilter()
        and count the same input: every k-mer that occurs twice is in the table with its exact count, one that occurs once
        is absent or, seldom, there with count 1.  The table is neither read nor written here."""
        self._prefilter_for(bits)
        b = bytes(text)
        _check(self._lib.tsx_hip_prefilter_add_host(self.handle, b, len(b), int(chunk_bytes)))

    def prefilterBgzf(self, gz, bits=None):
        """The same for the image of a blocked gzip (BGZF) file, inflated on the device (tsx_hip_prefilter_add_bgzf_host)."""
        self._prefilter_for(bits)
        b = bytes(gz)
        _check(self._lib.tsx_hip_prefilter_add_bgzf_host(self.handle, b, len(b)), refusal=True)

    def prefilterDevice(self, text_ptr, nbytes, bits=None, stream=None):
        """tsx_hip_prefilter_add_device: pass 1 over a device text (16-byte aligned).  Queued, not waited for (bits given:
        creating the filter waits for its zeroing first).  An armed count orders itself behind it, on any stream."""
        self._prefilter_for(bits)
        _check(self._lib.tsx_hip_prefilter_add_device(self.handle, _vp(text_ptr), nbytes, _stream(stream)))

    def armPrefilter(self, on=True):
        """While on, countFastq / countFastqDevice / countFastqBgzf insert only the windows the prefilter has seen twice
        (tsx_hip_prefilter_arm).  addKmers, load, combine and the read calls are not gated."""
        _check(self._lib.tsx_hip_prefilter_arm(self.handle, 1 if on else 0))

    @property
    def prefilter_bits(self):
        """The bits of the map's prefilter, 0 without one (tsx_hip_prefilter_bits: host state, no GPU call)."""
        return int(self._lib.tsx_hip_prefilter_bits(self.handle))

    @property
    def prefilter_stats(self):
        """{bits, seen, seen_again, admitted, skipped, set_bits_a, set_bits_b} (tsx_hip_prefilter_stats); all zero without
        a filter.  Waits for the map's work and counts the set bits of both filters on the GPU: not for a hot loop."""
        t = PrefilterTotals()
        _check(self._lib.tsx_hip_prefilter_stats(self.handle, ctypes.byref(t)))
        return t.as_dict()

    def prefilterWords(self, which):
        """The 64-bit words of filter 'a' (seen) or 'b' (seen again) as numpy uint64 (tsx_hip_prefilter_read)."""
        if which not in ("a", "b"):
            raise ValueError("which: 'a' or 'b', not %r" % (which,))
        bits = self.prefilter_bits
        if not bits:
            raise TSXException(EINVAL, "the map has no prefilter")
        out = np.zeros(1 << (bits - (6 if which == "a" else 8)), dtype=np.uint64)
        _check(self._lib.tsx_hip_prefilter_read(self.handle, 0 if which == "a" else 1, _p(out), out.size))
        return out

    def countTwice(self, text, bits=None):
        """Count `text` without its singletons: a new prefilter, pass 1, the armed count, disarmed again.  Returns
        prefilter_stats."""
        self.createPrefilter(min(max(self.l + 6, PREFILTER_BITS[0]), PREFILTER_BITS[-1]) if bits is None else bits)
        self.prefilter(text)
        self.armPrefilter(True)
        try:
            self.countFastq(text)
        finally:
            self.armPrefilter(False)
        return self.prefilter_stats

    # --- mate pairs ----------------------------------------------------------------------------------------------------------
    def _pairs(self, call, text1, text2, out1, out2, singles, chunk_bytes):
        """The common part of filterPairs / trimPairs: the four outputs opened (paths) or taken (fds), the call, the
        totals as a dict."""
        b1 = bytes(text1)
        b2 = None if text2 is None else bytes(text2)
        s1, s2 = singles
        if b2 is None and (out2 is not None or s2 is not None):
            raise ValueError("an interleaved text has one output and one singles output")
        if out1 is None or (b2 is not None and out2 is None):
            raise ValueError("the kept pairs need an output for each input text")
        with _fds(out1, out2, s1, s2) as fds:
            io, tot = PairIO(*fds), PairTotals()
            rc = call(b1, len(b1), b2, 0 if b2 is None else len(b2), ctypes.byref(io), int(chunk_bytes), ctypes.byref(tot))
        _check(rc)
        return tot.as_dict()

    def filterPairs(self, text1, text2, out1, out2=None, singles=(None, None), pairs="both", check_names=False, lower=2,
                    upper=None, min_in_range=0, fraction=1.0, invert=False, chunk_bytes=0):
        """The read filter over mate pairs (tsx_hip_filter_pairs_host): record i of text1 and record i of text2 are
        one pair (text2=None: text1 is interleaved).  pairs="both" keeps a pair when both mates pass the rule, "any"
        when one does; kept mates go to out1 / out2 (interleaved: both to out1), a mate that passes alone under "both"
        to its singles output (None drops it).  Outputs are paths (created or truncated) or open file descriptors.
        check_names compares the mates' names (pair_name).  Returns the totals as a dict (PairTotals)."""
        if pairs not in PAIR_MODES:
            raise ValueError("pairs must be one of %s, not %r" % (sorted(PAIR_MODES), pairs))
        rule = filter_rule(lower, upper, min_in_range, fraction, invert)
        return self._pairs(lambda b1, n1, b2, n2, io, chunk, tot: self._lib.tsx_hip_filter_pairs_host(
            self.handle, b1, n1, b2, n2, ctypes.byref(rule), PAIR_MODES[pairs], 1 if check_names else 0, io, chunk, tot),
            text1, text2, out1, out2, singles, chunk_bytes)

    def trimPairs(self, text1, text2, out1, out2=None, singles=(None, None), check_names=False, lower=2, upper=None,
                  mode="longest", min_len=0, chunk_bytes=0):
        """The trim over mate pairs (tsx_hip_trim_pairs_host): each mate is trimmed as trimReads trims it; a pair whose
        mates both survive goes to out1 / out2, a lone survivor to its singles output.  Arguments and result as
        filterPairs; the totals also count bases_in and bases_kept."""
        rule = trim_rule(lower, upper, mode, min_len)
        return self._pairs(lambda b1, n1, b2, n2, io, chunk, tot: self._lib.tsx_hip_trim_pairs_host(
            self.handle, b1, n1, b2, n2, ctypes.byref(rule), 1 if check_names else 0, io, chunk, tot),
            text1, text2, out1, out2, singles, chunk_bytes)

    # --- read calls on a device text -----------------------------------------------------------------------------------------
    def trimSpansDevice(self, text_ptr, nbytes, spans_ptr, cap, rule, stream=None):
        """tsx_hip_trim_spans_device: the kept spans of the records of a device text into a device buffer of cap spans.
        Returns the record count (more than cap: TSXException ERANGE)."""
        n = ctypes.c_size_t(0)
        _check(self._lib.tsx_hip_trim_spans_device(self.handle, _vp(text_ptr), nbytes, ctypes.byref(rule), _vp(spans_ptr), cap,
                                                   ctypes.byref(n), _stream(stream)))
        return int(n.value)

    def trimReadsDevice(self, text_ptr, nbytes, out_ptr, out_cap, rule, stream=None):
        """tsx_hip_trim_reads_device: the trimmed records of a device text into a device buffer.  Returns the totals."""
        tot = TrimTotals()
        _check(self._lib.tsx_hip_trim_reads_device(self.handle, _vp(text_ptr), nbytes, ctypes.byref(rule), _vp(out_ptr), out_cap,
                                                   ctypes.byref(tot), _stream(stream)))
        return tot.as_dict()

    def queryReadsDevice(self, text_ptr, nbytes, stats_ptr, cap, lower=1, upper=None, stream=None):
        """tsx_hip_query_reads_device: stats of the records of a device text into a device buffer of cap records.
        Returns the record count (more than cap: TSXException ERANGE)."""
        n = ctypes.c_size_t(0)
        _check(self._lib.tsx_hip_query_reads_device(self.handle, _vp(text_ptr), nbytes, int(lower), _upper(upper), _vp(stats_ptr),
                                                    cap, ctypes.byref(n), _stream(stream)))
        return int(n.value)

    def filterReadsDevice(self, text_ptr, nbytes, out_ptr, out_cap, rule, stream=None):
        """tsx_hip_filter_reads_device: the passing records of a device text into a device buffer.  Returns (records
        kept, bytes)."""
        nb, kept = ctypes.c_size_t(0), ctypes.c_uint64(0)
        _check(self._lib.tsx_hip_filter_reads_device(self.handle, _vp(text_ptr), nbytes, ctypes.byref(rule), _vp(out_ptr), out_cap,
                                                     ctypes.byref(nb), ctypes.byref(kept), _stream(stream)))
        return int(kept.value), int(nb.value)

    def getKmerCountsDevice(self, kmers_ptr, n, out_ptr, stream=None):
        _check(self._lib.tsx_hip_get_counts_device(self._h, _vp(kmers_ptr), n, _vp(out_ptr), _stream(stream)))

    def print_stats(self):
        s = self.stats()
        import sys
        print("Used fields: %d" % s["distinct"], file=sys.stderr)
        print("Available fields: %d" % self.getMaxElements(), file=sys.stderr)
        print("k=%d l=%d entry limbs=%d storage bits=%d" % (self.k, self.l, self.layout.entry_limbs,
                                                          self.layout.count_bits), file=sys.stderr)
        return s

    # --- counting path -----------------------------------------------------
    def countFastq(self, data):
        """countKMers (main.cpp:104-218) for one FASTQ text held in host memory."""
        b = bytes(data)
        _check(self._lib.tsx_hip_count_fastq_host(self._h, b, len(b)))

    def countFastqBgzf(self, gz):
        """The same for the image of a blocked gzip (BGZF) file: members inflated on the device (tsx_inflate.h)."""
        b = bytes(gz)
        _check(self._lib.tsx_hip_count_fastq_bgzf_host(self._h, b, len(b)), refusal=True)

    def countFastqDevice(self, dev_ptr, nbytes, stream=None):
        _check(self._lib.tsx_hip_count_fastq_device(self._h, _vp(dev_ptr), nbytes, _stream(stream)))

    def countFasta(self, data):
        """Count a wrapped (multi-line) FASTA text held in host memory: the sequence lines of a record are joined on the
        device (csrc/tsx_fasta.h), the k-mers are those of join_fasta(data) read as two-line records.  Works whatever
        set_record_lines says and leaves it alone."""
        b = bytes(data)
        _check(self._lib.tsx_hip_count_fasta_host(self.handle, b, len(b)), refusal=True)

    def countFastaBgzf(self, gz):
        """The same for the image of a blocked gzip (BGZF) file."""
        b = bytes(gz)
        _check(self._lib.tsx_hip_count_fasta_bgzf_host(self.handle, b, len(b)), refusal=True)

    def countFastaDevice(self, dev_ptr, nbytes, stream=None):
        """The same for a text resident on the device (16-byte aligned); queued, call sync() before reading."""
        _check(self._lib.tsx_hip_count_fasta_device(self.handle, _vp(dev_ptr), nbytes, _stream(stream)), refusal=True)

    def clear(self):
        _check(self._lib.tsx_hip_clear(self._h))

    def sync(self):
        _check(self._lib.tsx_hip_sync(self._h))

    def stats(self):
        s = Stats()
        _check(self._lib.tsx_hip_get_stats(self._h, ctypes.byref(s)))
        return s.as_dict()

    def set_timing(self, enable=True):
        _check(self._lib.tsx_hip_set_timing(self._h, 1 if enable else 0))

    def get_timing(self):
        """(line-pass ms, count_fastq_kernel ms, partition+build ms, pieces) since the last call."""
        a, b, c, n = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_double(0), ctypes.c_uint64(0)
        _check(self._lib.tsx_hip_get_timing(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c),
                                            ctypes.byref(n)))
        return a.value, b.value, c.value, int(n.value)

    def get_stage_timing(self):
        """({stage: ms}, pieces) since the last call; stages: line, scan, level1, level2, build, gap, post
        (gap = scan end to partition start: the owner split and the key exchange of a sharded run;
        post = overflow queues + deferred list, inserted after the build kernel)."""
        ms, n = (ctypes.c_double * 7)(), ctypes.c_uint64(0)
        _check(self._lib.tsx_hip_get_stage_timing(self._h, ms, ctypes.byref(n)))
        return dict(zip(("line", "scan", "level1", "level2", "build", "gap", "post"), [float(x) for x in ms])), int(n.value)

    def set_record_lines(self, lines):
        """4 = FASTQ records (default), 2 = FASTA as FASTXreader<FASTAEntry> reads it (tsx_hip_set_record_lines)."""
        if lines != 4 and self.base_rule[1] is not None:
            raise ValueError("min_qual_char needs FASTQ records: a FASTA text has no quality line")
        _check(self._lib.tsx_hip_set_record_lines(self._h, lines))
        self._lines = lines

    def set_path(self, path):
        """0 auto, 1 atomic, 2 partitioned (tsx_hip_set_path)."""
        _check(self._lib.tsx_hip_set_path(self._h, {"auto": 0, "atomic": 1, "partitioned": 2}.get(path, path)))

    # --- mapping -------------------------------------------------------------
    def hash_rows(self):
        out = np.zeros((2 * self.k, self.wk), dtype=np.uint64)
        _check(self._lib.tsx_hip_hash_rows(self._h, _p(out)))
        return out

    def hash_apply(self, kmer):
        a = np.ascontiguousarray(kmer, dtype=np.uint64)
        out = np.zeros(self.wk, dtype=np.uint64)
        _check(self._lib.tsx_hip_hash_apply(self._h, _p(a), _p(out)))
        return out

    def hash_invert(self, key):
        a = np.ascontiguousarray(key, dtype=np.uint64)
        out = np.zeros(self.wk, dtype=np.uint64)
        _check(self._lib.tsx_hip_hash_invert(self._h, _p(a), _p(out)))
        return out

    def owner(self, kmer, nranks):
        a = np.ascontiguousarray(kmer, dtype=np.uint64)
        return int(self._lib.tsx_hip_owner_host(self._h, _p(a), nranks))

    def _as_kmers(self, items):
        out = np.zeros((len(items), self.wk), dtype=np.uint64)
        for i, it in enumerate(items):
            out[i] = encode(it, self.k) if isinstance(it, (str, bytes)) else np.asarray(it, dtype=np.uint64)
        return out
