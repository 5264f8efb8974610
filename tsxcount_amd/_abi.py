"""The mirror of the C ABI (include/tsxcount_hip.h) and what every call through it shares: paths, error codes,
structures, dtypes, the rule builders, the signature table, the loader, the error check and the call helpers."""
import contextlib
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libtsxcount_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "tsxcount_hip.h")

OK, EINVAL, ENODEVICE, ENOMEM, EHIP, EFULL, EOVERFLOW, ERANGE, ELOCK, EIO = 0, -1, -2, -3, -4, -5, -6, -7, -8, -9
EFORMAT = -10
EPAIR = -11


class TSXException(RuntimeError):
    """Mirror of TSXException (TSXHashMap.h:28-47); carries the C-ABI code."""

    def __init__(self, code, what):
        super().__init__(what)
        self.code = code


# ---- structures ---------------------------------------------------------------------------------------------------------
class _Totals(ctypes.Structure):
    """A structure of plain integer fields that reads out as a dict."""

    def as_dict(self):
        return {f: int(getattr(self, f)) for f, _ in self._fields_}


class Layout(ctypes.Structure):
    _fields_ = [("k", ctypes.c_int32), ("l", ctypes.c_int32), ("key_limbs", ctypes.c_int32),
                ("entry_limbs", ctypes.c_int32), ("func_bits", ctypes.c_int32),
                ("reprobe_bits", ctypes.c_int32), ("count_bits", ctypes.c_int32),
                ("overflow_l", ctypes.c_int32), ("shard_bits", ctypes.c_int32), ("shard_index", ctypes.c_int32),
                ("max_reprobes", ctypes.c_uint32),
                ("slots", ctypes.c_uint64), ("table_bytes", ctypes.c_uint64)]


class Stats(_Totals):
    _fields_ = [("kmers_added", ctypes.c_uint64), ("insert_failures", ctypes.c_uint64),
                ("overflow_carries", ctypes.c_uint64), ("overflow_failures", ctypes.c_uint64),
                ("distinct", ctypes.c_uint64), ("overflow_used", ctypes.c_uint64),
                ("lock_timeouts", ctypes.c_uint64), ("fallback_inserts", ctypes.c_uint64),
                ("count_sum", ctypes.c_uint64)]


class FilterRule(ctypes.Structure):
    """tsx_hip_filter_rule: a record passes iff in_range >= min_in_range and in_range * 10^6 >= fraction_ppm * kmers."""
    _fields_ = [("lower", ctypes.c_uint64), ("upper", ctypes.c_uint64), ("min_in_range", ctypes.c_uint64),
                ("fraction_ppm", ctypes.c_uint32), ("invert", ctypes.c_int32)]


class TrimRule(ctypes.Structure):
    """tsx_hip_trim_rule: a window is solid when lower <= count <= upper; mode picks the run that is kept."""
    _fields_ = [("lower", ctypes.c_uint64), ("upper", ctypes.c_uint64), ("min_len", ctypes.c_uint64),
                ("mode", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class MedianRule(ctypes.Structure):
    """tsx_hip_median_rule: a record passes iff lower <= median <= upper; invert writes the failures."""
    _fields_ = [("lower", ctypes.c_uint64), ("upper", ctypes.c_uint64), ("invert", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


class NormalizeRule(ctypes.Structure):
    """tsx_hip_normalize_rule: a record is kept iff its median < cutoff; rounds of round_records records."""
    _fields_ = [("cutoff", ctypes.c_uint64), ("round_records", ctypes.c_uint64), ("reserved", ctypes.c_int32 * 2)]


class NormalizeTotals(_Totals):
    """tsx_hip_normalize_totals."""
    _fields_ = [(f, ctypes.c_uint64) for f in ("records", "kept", "kmers_seen", "kmers_added", "rounds")]


class TrimTotals(_Totals):
    """tsx_hip_trim_totals."""
    _fields_ = [("records", ctypes.c_uint64), ("kept", ctypes.c_uint64), ("bases_in", ctypes.c_uint64),
                ("bases_kept", ctypes.c_uint64), ("bytes", ctypes.c_uint64)]


class CorrectRule(ctypes.Structure):
    """tsx_hip_correct_rule: a window is solid when lower <= count <= upper; a run of fewer than min_windows is no site."""
    _fields_ = [("lower", ctypes.c_uint64), ("upper", ctypes.c_uint64), ("min_windows", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


class CorrectTotals(_Totals):
    """tsx_hip_correct_totals."""
    _fields_ = [(f, ctypes.c_uint64) for f in ("records", "sites", "corrected", "ambiguous", "unfixable", "bytes")]


class UnitigRule(ctypes.Structure):
    """tsx_hip_unitig_rule: a k-mer is a node when lower <= count <= upper; flags must be 0."""
    _fields_ = [("lower", ctypes.c_uint64), ("upper", ctypes.c_uint64), ("flags", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class UnitigTotals(ctypes.Structure):
    """tsx_hip_unitig_totals; degree[5 * in + out] counts the nodes by in- and out-degree."""
    _fields_ = [(f, ctypes.c_uint64) for f in ("nodes", "unitigs", "circular", "bases", "longest", "isolated", "tips",
                                               "branching", "sum_count")] + [("degree", ctypes.c_uint64 * 25)]

    def as_dict(self):
        d = {f: int(getattr(self, f)) for f, _ in self._fields_[:-1]}
        d["degree"] = [int(v) for v in self.degree]
        return d


class PairIO(ctypes.Structure):
    """tsx_hip_pair_io: the four outputs of a pair call (-1 = none)."""
    _fields_ = [("fd1", ctypes.c_int), ("fd2", ctypes.c_int), ("fd_single1", ctypes.c_int), ("fd_single2", ctypes.c_int)]


class PairTotals(_Totals):
    """tsx_hip_pair_totals."""
    _fields_ = [(f, ctypes.c_uint64) for f in ("pairs", "kept", "single1", "single2", "bytes1", "bytes2", "bytes_single1",
                                               "bytes_single2", "bases_in", "bases_kept")]


class SketchTotals(_Totals):
    """tsx_hip_sketch_totals: what a sketch call saw."""
    _fields_ = [("kmers", ctypes.c_uint64), ("records", ctypes.c_uint64)]


class PrefilterTotals(_Totals):
    """tsx_hip_prefilter_totals: the size of a map's prefilter, what its two passes saw, its fill."""
    _fields_ = [(n, ctypes.c_uint64) for n in ("bits", "seen", "seen_again", "admitted", "skipped", "set_bits_a", "set_bits_b")]


class Level1Shape(ctypes.Structure):
    """tsx_hip_level1_shape: the level-1 sub-lists the last plain partitioned count of a map left."""
    _fields_ = [("nb", ctypes.c_uint32), ("G", ctypes.c_uint32), ("cpr2", ctypes.c_uint32), ("wg_major", ctypes.c_int),
                ("cap", ctypes.c_uint64)]


class DbInfo(_Totals):
    """tsx_hip_db_info: the header of a k-mer database file."""
    _fields_ = [("version", ctypes.c_uint32), ("k", ctypes.c_int32), ("l", ctypes.c_int32),
                ("entry_limbs", ctypes.c_int32), ("func_bits", ctypes.c_int32), ("reprobe_bits", ctypes.c_int32),
                ("count_bits", ctypes.c_int32), ("seg_bits", ctypes.c_int32), ("overflow_l", ctypes.c_int32),
                ("canonical", ctypes.c_int32), ("acgt_only", ctypes.c_int32), ("min_qual_char", ctypes.c_int32),
                ("hash_seed", ctypes.c_uint64), ("kmers_added", ctypes.c_uint64), ("distinct", ctypes.c_uint64),
                ("count_sum", ctypes.c_uint64), ("carry_records", ctypes.c_uint64)]


class CombineRule(ctypes.Structure):
    """tsx_hip_combine_rule: the op, the count mode and the count range of each input."""
    _fields_ = [("op", ctypes.c_int32), ("count_mode", ctypes.c_int32), ("a_lower", ctypes.c_uint64),
                ("a_upper", ctypes.c_uint64), ("b_lower", ctypes.c_uint64), ("b_upper", ctypes.c_uint64)]


class CombineStats(_Totals):
    """tsx_hip_combine_stats."""
    _fields_ = [("a_in_range", ctypes.c_uint64), ("b_in_range", ctypes.c_uint64), ("both", ctypes.c_uint64),
                ("a_sum_both", ctypes.c_uint64), ("b_sum_both", ctypes.c_uint64), ("out_entries", ctypes.c_uint64),
                ("out_count_sum", ctypes.c_uint64)]


class HetRule(ctypes.Structure):
    """tsx_hip_het_rule"""
    _fields_ = [("lower", ctypes.c_uint64), ("upper", ctypes.c_uint64), ("mode", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class HetStats(ctypes.Structure):
    """tsx_hip_het_stats"""
    _fields_ = [(n, ctypes.c_uint64) for n in ("kmers_in_range", "paired", "pairs", "families_2", "families_3plus")]


class BinRule(ctypes.Structure):
    """tsx_hip_bin_rule."""
    _fields_ = [("a_lower", ctypes.c_uint64), ("a_upper", ctypes.c_uint64), ("b_lower", ctypes.c_uint64),
                ("b_upper", ctypes.c_uint64), ("min_hits", ctypes.c_uint64), ("ratio_milli", ctypes.c_uint32),
                ("reserved", ctypes.c_int32)]


class BinIO(ctypes.Structure):
    """tsx_hip_bin_io: one file descriptor per class, -1 = counted and not written."""
    _fields_ = [("fd_a", ctypes.c_int), ("fd_b", ctypes.c_int), ("fd_ambiguous", ctypes.c_int), ("fd_none", ctypes.c_int)]


class BinTotals(ctypes.Structure):
    """tsx_hip_bin_totals."""
    _fields_ = [("records", ctypes.c_uint64), ("n", ctypes.c_uint64 * 4), ("bytes", ctypes.c_uint64 * 4)]

    def as_dict(self):
        return {"records": int(self.records), "n": [int(v) for v in self.n], "bytes": [int(v) for v in self.bytes]}


# ---- constants and record dtypes ------------------------------------------------------------------------------------------
NORMALIZE_ROUND = 65536   # TSX_HIP_NORMALIZE_ROUND: part of the result's definition
COMBINE_OPS = {"intersect": 0, "union": 1, "subtract": 2, "diff": 3}
COMBINE_COUNTS = {"min": 0, "max": 1, "sum": 2, "left": 3, "right": 4}
TRIM_MODES = {"longest": 0, "prefix": 1}
PAIR_MODES = {"both": 0, "any": 1}
HET_MODES = {"unique": 0, "all": 1}
NO_KMER = 0xFFFFFFFF          # TSX_HIP_NO_KMER: the profile entry of a position where no k-mer starts
SKETCH_PRECISIONS = range(10, 15)   # the p of a sketch: 2^p registers
PREFILTER_BITS = range(12, 39)    # a prefilter's size: filter A has 2^bits bits, filter B 2^(bits - 2)
JOINT_MAX_CELLS = 1 << 24   # cells of a joint histogram (tsx_hip_joint_histogram_*)
BIN_A, BIN_B, BIN_AMBIGUOUS, BIN_NONE = 0, 1, 2, 3   # TSX_HIP_BIN_*: the class of a record
BIN_NAMES = ("a", "b", "ambiguous", "none")
SEQ_NAME_MAX = 255

READ_STATS_DTYPE = np.dtype([("kmers", np.uint64), ("in_range", np.uint64), ("min_count", np.uint64), ("sum_count", np.uint64)])
TRIM_SPAN_DTYPE = np.dtype([("start", np.uint64), ("length", np.uint64)])
READ_MEDIAN_DTYPE = np.dtype([("kmers", np.uint64), ("median", np.uint64)])
BIN_STATS_DTYPE = np.dtype([("kmers", np.uint64), ("hits_a", np.uint64), ("hits_b", np.uint64), ("hits_both", np.uint64)])
SEQ_STATS_DTYPE = np.dtype([("length", np.uint64), ("kmers", np.uint64), ("present", np.uint64), ("min_count", np.uint64),
                            ("sum_count", np.uint64)])
SEQ_INTERVAL_DTYPE = np.dtype([("seq", np.uint64), ("start", np.uint64), ("end", np.uint64)])


def key_limbs(k):
    return (2 * k + 63) // 64


def het_pair_dtype(k):
    """A record of the pair list of a table of k-mers (tsx_hip_het_pairs_device): k-mers as key_limbs(k) limbs."""
    w = key_limbs(k)
    return np.dtype([("minor", np.uint64, (w,)), ("major", np.uint64, (w,)), ("minor_count", np.uint64), ("major_count", np.uint64)])


HET_PAIR_DTYPE = het_pair_dtype(31)   # one-limb keys (k <= 32); het_pair_dtype(k) for any k


# ---- rule builders --------------------------------------------------------------------------------------------------------
def _upper(upper):
    """The upper end of a count range: None = no bound."""
    return (1 << 64) - 1 if upper is None else int(upper)


def filter_rule(lower=2, upper=None, min_in_range=0, fraction=1.0, invert=False):
    """A FilterRule from the Python arguments (fraction: share of a record's k-mers that must be in range, 0..1)."""
    return FilterRule(int(lower), _upper(upper), int(min_in_range), int(round(float(fraction) * 1e6)), 1 if invert else 0)


def trim_rule(lower=2, upper=None, mode="longest", min_len=0):
    """A TrimRule from the Python arguments (mode by name, TRIM_MODES).  Raises ValueError for an unknown mode and for
    lower > upper, before any GPU call."""
    if mode not in TRIM_MODES:
        raise ValueError("trim mode must be one of %s, not %r" % (sorted(TRIM_MODES), mode))
    upper = _upper(upper)
    if int(lower) > upper:
        raise ValueError("trim range: lower %d > upper %d" % (int(lower), upper))
    return TrimRule(int(lower), upper, int(min_len), TRIM_MODES[mode], 0)


def median_rule(lower=0, upper=None, invert=False):
    """A MedianRule from the Python arguments.  Raises ValueError for lower > upper, before any GPU call."""
    upper = _upper(upper)
    if int(lower) > upper:
        raise ValueError("median range: lower %d > upper %d" % (int(lower), upper))
    return MedianRule(int(lower), upper, 1 if invert else 0, 0)


def normalize_rule(cutoff=20, round_records=NORMALIZE_ROUND):
    """A NormalizeRule from the Python arguments.  Raises ValueError for round_records < 1, before any GPU call."""
    if int(round_records) < 1:
        raise ValueError("normalize: round_records %d < 1" % int(round_records))
    if int(cutoff) < 0:
        raise ValueError("normalize: cutoff %d < 0" % int(cutoff))
    return NormalizeRule(min(int(cutoff), (1 << 64) - 1), int(round_records), (ctypes.c_int32 * 2)(0, 0))


def combine_rule(op="intersect", counts="min", a_range=(1, None), b_range=(1, None)):
    """A CombineRule from the Python arguments: op and counts by name (COMBINE_OPS, COMBINE_COUNTS) or number, each
    range as (lower, upper) with None = no upper bound."""
    return CombineRule(int(COMBINE_OPS.get(op, op)), int(COMBINE_COUNTS.get(counts, counts)),
                       int(a_range[0]), _upper(a_range[1]), int(b_range[0]), _upper(b_range[1]))


def het_rule(lower=1, upper=None, mode="unique"):
    if mode not in HET_MODES:
        raise ValueError("het pairs: mode is 'unique' or 'all', got %r" % (mode,))
    return HetRule(int(lower), _upper(upper), HET_MODES[mode], 0)


def bin_rule(a_range=(1, None), b_range=(1, None), min_hits=1, ratio=1.0):
    """A BinRule from the Python arguments: each range as (lower, upper) with None = no upper bound, the ratio as a
    number >= 1 (three decimal places kept)."""
    return BinRule(int(a_range[0]), _upper(a_range[1]), int(b_range[0]), _upper(b_range[1]),
                   int(min_hits), min(max(int(round(float(ratio) * 1000)), 0), (1 << 32) - 1), 0)


# ---- the signatures: every function include/tsxcount_hip.h declares, as (restype, argtypes) -------------------------------
def _signatures():
    P = ctypes.POINTER
    ci, sz, u32, u64, dbl = ctypes.c_int, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_double
    vp, ccp = ctypes.c_void_p, ctypes.c_char_p
    cip, szp, u8p, u32p, u64p, dblp, vpp = P(ci), P(sz), P(ctypes.c_uint8), P(u32), P(u64), P(dbl), P(vp)
    return {
        "tsx_hip_strerror": (ccp, [ci]),
        "tsx_hip_last_error": (ccp, []),
        "tsx_hip_device_count": (ci, []),
        "tsx_hip_key_limbs": (ci, [ci]),
        "tsx_hip_encode": (ci, [ccp, ci, u64p]),
        "tsx_hip_decode": (ci, [u64p, ci, ccp]),
        "tsx_hip_create": (ci, [vpp, ci, ci, ci, ci, u64, ci]),
        "tsx_hip_create_shard": (ci, [vpp, ci, ci, ci, ci, u64, ci, ci, ci]),
        "tsx_hip_shard_send_capacity": (ci, [vp, sz, szp]),
        "tsx_hip_shard_scan_device": (ci, [vp, vp, sz, vp, sz, vp, vp, vp, sz, vp, vp]),
        "tsx_hip_shard_scan_window_device": (ci, [vp, vp, sz, sz, sz, vp, sz, vp, sz, vp, vp, vp, sz, vp, vp, vp]),
        "tsx_hip_shard_build_device": (ci, [vp, vp, sz, vp, vp]),
        "tsx_hip_shard_build_pieces_device": (ci, [vp, vp, u64p, u64p, sz, vp, vp]),
        "tsx_hip_add_hashed_device": (ci, [vp, vp, vp, sz, vp]),
        "tsx_hip_bgzf_index_host": (ci, [vp, sz, szp, szp]),
        "tsx_hip_inflate_bgzf_host": (ci, [ci, vp, sz, vp, sz, szp]),
        "tsx_hip_count_fastq_bgzf_host": (ci, [vp, vp, sz]),
        "tsx_hip_shard_l1_supported": (ci, [vp]),
        "tsx_hip_shard_l1_window_device": (ci, [vp, vp, sz, u32, u32, sz, vp, vp]),
        "tsx_hip_shard_build_l1_device": (ci, [vp, vp]),
        "tsx_hip_shard_desc_capacity": (ci, [vp, sz, ci, szp]),
        "tsx_hip_shard_desc_window_device": (ci, [vp, vp, sz, sz, sz, ci, vp, sz, vp, vp, vp]),
        "tsx_hip_shard_walk_device": (ci, [vp, vp, sz, ci, u32, u32, sz, vp, vp]),
        "tsx_hip_shard_filter_device": (ci, [vp, vp, sz, ci, u32, u32, sz, vp, vp]),
        "tsx_hip_mini_supported": (ci, [vp]),
        "tsx_hip_mini_capacity": (ci, [vp, sz, ci, szp]),
        "tsx_hip_mini_window_device": (ci, [vp, vp, sz, sz, sz, ci, vp, sz, vp, vp, vp]),
        "tsx_hip_mini_part_capacity": (ci, [vp, sz, u32, szp]),
        "tsx_hip_mini_describe_device": (ci, [vp, vp, sz, sz, sz, vp, vp]),
        "tsx_hip_mini_split_device": (ci, [vp, u32, u32, ci, vp, sz, vp, vp]),
        "tsx_hip_mini_owner_host": (ci, [ci, ci, u64p, sz, u32p]),
        "tsx_hip_destroy": (None, [vp]),
        "tsx_hip_get_layout": (ci, [vp, P(Layout)]),
        "tsx_hip_clear": (ci, [vp]),
        "tsx_hip_set_canonical": (ci, [vp, ci]),
        "tsx_hip_canonical": (ci, [vp]),
        "tsx_hip_canonical_host": (ci, [ci, u64p, sz, u64p]),
        "tsx_hip_group_set_canonical": (ci, [vp, ci]),
        "tsx_hip_set_base_rule": (ci, [vp, ci, ci]),
        "tsx_hip_get_base_rule": (ci, [vp, cip, cip]),
        "tsx_hip_group_set_base_rule": (ci, [vp, ci, ci]),
        "tsx_hip_sync": (ci, [vp]),
        "tsx_hip_count_fastq_host": (ci, [vp, ccp, sz]),
        "tsx_hip_count_fastq_device": (ci, [vp, vp, sz, vp]),
        "tsx_hip_count_fasta_host": (ci, [vp, ccp, sz]),
        "tsx_hip_count_fasta_device": (ci, [vp, vp, sz, vp]),
        "tsx_hip_count_fasta_bgzf_host": (ci, [vp, vp, sz]),
        "tsx_hip_unwrap_fasta_host": (ci, [ci, ccp, sz, vp, sz, szp]),
        "tsx_hip_add_kmers_host": (ci, [vp, u64p, u64p, sz]),
        "tsx_hip_add_kmers_device": (ci, [vp, vp, vp, sz, vp]),
        "tsx_hip_get_counts_host": (ci, [vp, u64p, sz, u64p]),
        "tsx_hip_get_counts_device": (ci, [vp, vp, sz, vp, vp]),
        "tsx_hip_lookup_host": (ci, [vp, u64p, sz, u64p, u64p]),
        "tsx_hip_kmer_starts_host": (ci, [vp, u8p, sz]),
        "tsx_hip_get_stats": (ci, [vp, P(Stats)]),
        "tsx_hip_dump_host": (ci, [vp, u64p, u64p, sz, szp]),
        "tsx_hip_dump_device": (ci, [vp, vp, vp, sz, vp, vp]),
        "tsx_hip_partition_device": (ci, [vp, ci, vp, vp, sz, vp, vp]),
        "tsx_hip_dump_range_device": (ci, [vp, u64, u64, vp, vp, sz, vp, vp]),
        "tsx_hip_owner_host": (ci, [vp, u64p, ci]),
        "tsx_hip_histogram_device": (ci, [vp, u64, u64, sz, vp, vp]),
        "tsx_hip_histogram_host": (ci, [vp, u64p, sz]),
        "tsx_hip_format_counts_device": (ci, [vp, u64, u64, u64, u64, vp, sz, vp, vp, vp]),
        "tsx_hip_write_counts_host": (ci, [vp, ci, u64, u64, sz, u64p, u64p]),
        "tsx_hip_db_read_info": (ci, [ci, P(DbInfo)]),
        "tsx_hip_save_host": (ci, [vp, ci, sz, u64p, u64p]),
        "tsx_hip_load_host": (ci, [vp, ci, sz, u64p]),
        "tsx_hip_combine": (ci, [vp, vp, vp, P(CombineRule), P(CombineStats)]),
        "tsx_hip_joint_histogram_device": (ci, [vp, vp, sz, sz, vp, vp]),
        "tsx_hip_joint_histogram_host": (ci, [vp, vp, u64p, sz, sz]),
        "tsx_hip_het_histogram_device": (ci, [vp, P(HetRule), sz, sz, vp, vp, vp]),
        "tsx_hip_het_histogram_host": (ci, [vp, P(HetRule), u64p, sz, sz, P(HetStats)]),
        "tsx_hip_het_pairs_device": (ci, [vp, P(HetRule), u64, u64, vp, sz, vp, vp]),
        "tsx_hip_write_het_pairs_host": (ci, [vp, P(HetRule), ci, sz, u64p, u64p]),
        "tsx_hip_bin_stats_device": (ci, [vp, vp, vp, sz, P(BinRule), vp, sz, szp, vp]),
        "tsx_hip_bin_stats_host": (ci, [vp, vp, ccp, sz, P(BinRule), vp, vp, sz, szp, sz]),
        "tsx_hip_bin_reads_host": (ci, [vp, vp, ccp, sz, P(BinRule), P(BinIO), sz, P(BinTotals)]),
        "tsx_hip_group_histogram_host": (ci, [vp, u64p, sz]),
        "tsx_hip_group_write_counts_host": (ci, [vp, ci, u64, u64, sz, u64p, u64p]),
        "tsx_hip_query_reads_device": (ci, [vp, vp, sz, u64, u64, vp, sz, szp, vp]),
        "tsx_hip_query_reads_host": (ci, [vp, ccp, sz, u64, u64, vp, sz, szp, sz]),
        "tsx_hip_filter_reads_host": (ci, [vp, ccp, sz, P(FilterRule), ci, sz, u64p, u64p]),
        "tsx_hip_filter_reads_device": (ci, [vp, vp, sz, P(FilterRule), vp, sz, szp, u64p, vp]),
        "tsx_hip_trim_spans_device": (ci, [vp, vp, sz, P(TrimRule), vp, sz, szp, vp]),
        "tsx_hip_trim_spans_host": (ci, [vp, ccp, sz, P(TrimRule), vp, sz, szp, sz]),
        "tsx_hip_trim_reads_device": (ci, [vp, vp, sz, P(TrimRule), vp, sz, P(TrimTotals), vp]),
        "tsx_hip_trim_reads_host": (ci, [vp, ccp, sz, P(TrimRule), ci, sz, P(TrimTotals)]),
        "tsx_hip_count_profile_device": (ci, [vp, vp, sz, vp, vp]),
        "tsx_hip_count_profile_host": (ci, [vp, ccp, sz, vp, sz]),
        "tsx_hip_median_reads_device": (ci, [vp, vp, sz, vp, sz, szp, vp]),
        "tsx_hip_median_reads_host": (ci, [vp, ccp, sz, vp, sz, szp, sz]),
        "tsx_hip_filter_median_host": (ci, [vp, ccp, sz, P(MedianRule), ci, sz, u64p, u64p]),
        "tsx_hip_normalize_host": (ci, [vp, ccp, sz, P(NormalizeRule), ci, vp, sz, sz, P(NormalizeTotals)]),
        "tsx_hip_normalize_device": (ci, [vp, vp, sz, P(NormalizeRule), vp, sz, P(NormalizeTotals), vp]),
        "tsx_hip_sketch_host": (ci, [vp, ccp, sz, ci, u8p, P(SketchTotals), sz]),
        "tsx_hip_sketch_bgzf_host": (ci, [vp, vp, sz, ci, u8p, P(SketchTotals)]),
        "tsx_hip_sketch_device": (ci, [vp, vp, sz, ci, vp, vp, vp]),
        "tsx_hip_sketch_kmers_host": (ci, [ci, u64p, sz, ci, u8p]),
        "tsx_hip_sketch_estimate_host": (dbl, [u8p, ci]),
        "tsx_hip_suggest_l": (ci, [ci, dbl, ci, u32, cip]),
        "tsx_hip_prefilter_create": (ci, [vp, ci]),
        "tsx_hip_prefilter_free": (ci, [vp]),
        "tsx_hip_prefilter_add_host": (ci, [vp, ccp, sz, sz]),
        "tsx_hip_prefilter_add_bgzf_host": (ci, [vp, vp, sz]),
        "tsx_hip_prefilter_add_device": (ci, [vp, vp, sz, vp]),
        "tsx_hip_prefilter_arm": (ci, [vp, ci]),
        "tsx_hip_prefilter_armed": (ci, [vp]),
        "tsx_hip_prefilter_bits": (ci, [vp]),
        "tsx_hip_prefilter_stats": (ci, [vp, P(PrefilterTotals)]),
        "tsx_hip_prefilter_read": (ci, [vp, ci, u64p, sz]),
        "tsx_hip_prefilter_mask_host": (ci, [ci, u64p, ci, u64p, u64p, u64p]),
        "tsx_hip_filter_pairs_host": (ci, [vp, ccp, sz, ccp, sz, P(FilterRule), ci, ci, P(PairIO), sz, P(PairTotals)]),
        "tsx_hip_correct_sites_device": (ci, [vp, vp, sz, P(CorrectRule), vp, sz, szp, P(CorrectTotals), vp]),
        "tsx_hip_correct_sites_host": (ci, [vp, ccp, sz, P(CorrectRule), vp, sz, szp, P(CorrectTotals), sz]),
        "tsx_hip_correct_reads_device": (ci, [vp, vp, sz, P(CorrectRule), vp, sz, P(CorrectTotals), vp]),
        "tsx_hip_correct_reads_host": (ci, [vp, ccp, sz, P(CorrectRule), ci, sz, P(CorrectTotals)]),
        "tsx_hip_unitig_stats": (ci, [vp, P(UnitigRule), P(UnitigTotals)]),
        "tsx_hip_unitigs_device": (ci, [vp, P(UnitigRule), vp, sz, vp, sz, szp, szp, P(UnitigTotals), vp]),
        "tsx_hip_unitigs_host": (ci, [vp, P(UnitigRule), vp, sz, vp, sz, szp, szp, P(UnitigTotals)]),
        "tsx_hip_write_unitigs_host": (ci, [vp, P(UnitigRule), ci, P(UnitigTotals)]),
        "tsx_hip_unitig_last_timing": (ci, [dblp]),
        "tsx_hip_trim_pairs_host": (ci, [vp, ccp, sz, ccp, sz, P(TrimRule), ci, P(PairIO), sz, P(PairTotals)]),
        "tsx_hip_hash_apply": (ci, [vp, u64p, u64p]),
        "tsx_hip_hash_invert": (ci, [vp, u64p, u64p]),
        "tsx_hip_hash_rows": (ci, [vp, u64p]),
        "tsx_hip_lut4_host": (ci, [ci, ci, u64, u64p]),
        "tsx_hip_sublist_first": (u64, [u32, u32, ci, u32, u32, u64]),
        "tsx_hip_level1_sizes_host": (ci, [vp, P(Level1Shape), u64p, sz]),
        "tsx_hip_set_timing": (ci, [vp, ci]),
        "tsx_hip_get_timing": (ci, [vp, dblp, dblp, dblp, u64p]),
        "tsx_hip_get_stage_timing": (ci, [vp, dblp, u64p]),
        "tsx_hip_set_path": (ci, [vp, ci]),
        "tsx_hip_set_record_lines": (ci, [vp, ci]),
        "tsx_hip_synth_fastq_device": (ci, [u64, u64, u64, ci, vp, sz, u64p, u64p, u64p, ci, vp]),
        "tsx_hip_synth_zipf_device": (ci, [u64, u64, u32, u32, u64p, vp, sz, u64p, ci, vp]),
        "tsx_hip_group_create": (ci, [vpp, ci, cip, ci, ci, ci, ci, u64, ci]),
        "tsx_hip_group_destroy": (None, [vp]),
        "tsx_hip_group_size": (ci, [vp]),
        "tsx_hip_group_map": (vp, [vp, ci]),
        "tsx_hip_group_comm_name": (ccp, [vp]),
        "tsx_hip_group_last_error": (ccp, []),
        "tsx_hip_group_set_record_lines": (ci, [vp, ci]),
        "tsx_hip_group_clear": (ci, [vp]),
        "tsx_hip_group_count_fastq_host": (ci, [vp, ccp, sz]),
        "tsx_hip_group_merge": (ci, [vp]),
        "tsx_hip_group_get_counts_host": (ci, [vp, u64p, sz, u64p]),
        "tsx_hip_group_get_stats": (ci, [vp, P(Stats)]),
        "tsx_hip_group_exchanged_entries": (u64, [vp]),
        "tsx_hip_group_set_exchange": (ci, [vp, ci]),
        "tsx_hip_group_exchange": (ci, [vp]),
        "tsx_hip_group_exchange_rounds": (u32, [vp]),
        "tsx_hip_cut_records_host": (ci, [ccp, sz, ci, ci, szp]),
        "tsx_hip_seq_stats_host": (ci, [vp, ccp, sz, u64, u64, sz, vpp]),
        "tsx_hip_seq_missing_host": (ci, [vp, ccp, sz, u64, u64, sz, vpp]),
        "tsx_hip_seq_stats_bgzf_host": (ci, [vp, vp, sz, u64, u64, vpp]),
        "tsx_hip_seq_missing_bgzf_host": (ci, [vp, vp, sz, u64, u64, vpp]),
        "tsx_hip_seq_stats_device": (ci, [vp, vp, sz, u64, u64, vpp, vp]),
        "tsx_hip_seq_missing_device": (ci, [vp, vp, sz, u64, u64, vpp, vp]),
        "tsx_hip_seq_result_count": (sz, [vp]),
        "tsx_hip_seq_result_stats": (vp, [vp]),
        "tsx_hip_seq_result_names": (vp, [vp, vpp]),
        "tsx_hip_seq_result_intervals": (sz, [vp, vpp]),
        "tsx_hip_seq_result_free": (None, [vp]),
        "tsx_hip_seq_write_stats": (ci, [vp, ci, ci]),
        "tsx_hip_seq_write_missing": (ci, [vp, ci]),
        "tsx_hip_seq_track_host": (ci, [vp, ccp, sz, u64, u64, u64, sz, vpp]),
        "tsx_hip_seq_track_bgzf_host": (ci, [vp, vp, sz, u64, u64, u64, vpp]),
        "tsx_hip_seq_track_device": (ci, [vp, vp, sz, u64, u64, u64, vpp, vp]),
        "tsx_hip_seq_result_bins": (sz, [vp, vpp, vpp]),
        "tsx_hip_seq_result_window": (u64, [vp]),
        "tsx_hip_seq_write_track": (ci, [vp, ci]),
    }


SIGNATURES = _signatures()


def build():
    """Compile the library in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    import subprocess
    subprocess.check_call(["make", "-C", os.path.join(_HERE, "csrc"), "all"], stdout=subprocess.DEVNULL)


_lib = None


def lib():
    """Load libtsxcount_hip.so with SIGNATURES applied; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("tsxcount_amd: %s is missing; run tsxcount_amd.build() "
                              "(hipcc --offload-arch=gfx950). There is no CPU fallback." % LIB_PATH)
        L = ctypes.CDLL(LIB_PATH)
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        _lib = L
    return _lib


# ---- what the calls share ---------------------------------------------------------------------------------------------------
def _check(code, refusal=False):
    """Raises TSXException for a code other than OK, with the library's words for it.  refusal: the call is one that
    says which argument or input it turned down (tsx_hip_last_error), and that text is the message of an EINVAL."""
    if code == OK:
        return
    L = lib()
    msg = L.tsx_hip_strerror(code).decode()
    if refusal and code == EINVAL:
        msg = L.tsx_hip_last_error().decode() or msg
    elif code in (EHIP, ENODEVICE, ENOMEM, EIO, EFORMAT, EPAIR):
        extra = L.tsx_hip_last_error().decode()
        if extra:
            msg += " (" + extra + ")"
    raise TSXException(code, msg)


def _p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))


def _stream(stream):
    """A stream argument: the handle as a pointer, None = the map's own stream."""
    return ctypes.c_void_p(stream) if stream else None


@contextlib.contextmanager
def _fds(*targets, read=False):
    """The file descriptors of the targets of a call, as a list: a path is opened (created or truncated; read: read-only),
    an int is the caller's descriptor and is taken as it is, None is -1 (no output).  Closes what it opened, and only
    that, also when a later open or the call raises."""
    flags = os.O_RDONLY if read else os.O_WRONLY | os.O_CREAT | os.O_TRUNC
    opened, fds = [], []
    try:
        for t in targets:
            if t is None or isinstance(t, int):
                fds.append(-1 if t is None else t)
            else:
                opened.append(os.open(t, flags, 0o644))
                fds.append(opened[-1])
        yield fds
    finally:
        for fd in opened:
            os.close(fd)


def _fetch_records(dtype, text_len, call, refusal=False):
    """One record per record of a text of text_len bytes, as a numpy array of dtype: call(out_ptr, cap, n_ref) -> code
    fills at most cap records and reports their number.  The first capacity is a guess from the text's length; when
    the library answers ERANGE the call is made once more with room for the number it reported."""
    cap = text_len // 256 + 16
    for _ in range(2):
        out = np.zeros(cap, dtype=dtype)
        n = ctypes.c_size_t(0)
        rc = call(out.ctypes.data_as(ctypes.c_void_p), cap, ctypes.byref(n))
        if rc != ERANGE:
            break
        cap = n.value
    _check(rc, refusal)
    return out[:n.value]


def _write_counts(fn, handle, check, path_or_fd, lower, upper, chunk_bytes):
    """tsx_hip_write_counts_host / tsx_hip_group_write_counts_host to a path (created or truncated) or a descriptor."""
    lines, nbytes = ctypes.c_uint64(0), ctypes.c_uint64(0)
    with _fds(path_or_fd) as (fd,):
        rc = fn(handle, fd, int(lower), _upper(upper), int(chunk_bytes), ctypes.byref(lines), ctypes.byref(nbytes))
    check(rc)
    return int(lines.value), int(nbytes.value)


# ---- k-mers as limbs (host-only entry points) ---------------------------------------------------------------------------------
def encode(seq, k=None):
    """TSXSeqUtils::fromSequence (SequenceUtils.h:86-160) -> uint64 limbs."""
    s = seq.encode() if isinstance(seq, str) else bytes(seq)
    k = len(s) if k is None else k
    out = np.zeros(key_limbs(k), dtype=np.uint64)
    _check(lib().tsx_hip_encode(s, k, _p(out)))
    return out


def decode(limbs, k):
    """TSXSeqUtils::toSequence (SequenceUtils.h:47-84)."""
    a = np.ascontiguousarray(limbs, dtype=np.uint64)
    buf = ctypes.create_string_buffer(k + 1)
    _check(lib().tsx_hip_decode(_p(a), k, buf))
    return buf.value.decode()


def encode_many(seqs, k):
    out = np.zeros((len(seqs), key_limbs(k)), dtype=np.uint64)
    for i, s in enumerate(seqs):
        out[i] = encode(s, k)
    return out


_COMP = str.maketrans("ACGT", "TGCA")


def revcomp(seq):
    """Reverse complement of an ACGT string (other bytes: see canonical())."""
    return seq[::-1].translate(_COMP)


def canonical(kmers, k):
    """The lexicographically smaller of each k-mer and its reverse complement (A < C < G < T), what a canonical
    table's dump reports.  A string gives a string; encoded limbs ((n, key_limbs) or flat) give limbs
    (tsx_hip_canonical_host: the complement is taken on the 2-bit code, so any byte has one)."""
    if isinstance(kmers, (str, bytes)):
        return decode(canonical(encode(kmers, k), k), k)
    a = np.ascontiguousarray(kmers, dtype=np.uint64)
    out = np.zeros_like(a)
    n = a.size // key_limbs(k)
    _check(lib().tsx_hip_canonical_host(k, _p(a), n, _p(out)))
    return out


def min_qual_code(min_qual_char):
    """The byte of a min_qual_char argument: None or 0 = off, a one-character str (e.g. '5') or an int 1 .. 255."""
    if min_qual_char is None:
        return 0
    if isinstance(min_qual_char, (bytes, str)):
        b = min_qual_char.encode("latin-1") if isinstance(min_qual_char, str) else min_qual_char
        if len(b) != 1:
            raise ValueError("min_qual_char: one character, got %r" % (min_qual_char,))
        return b[0]
    if isinstance(min_qual_char, bool) or not isinstance(min_qual_char, (int, np.integer)):
        raise TypeError("min_qual_char: a one-character str or an int, got %r" % (min_qual_char,))
    if not 0 <= int(min_qual_char) <= 255:
        raise ValueError("min_qual_char: 0 .. 255, got %d" % min_qual_char)
    return int(min_qual_char)
