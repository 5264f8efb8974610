"""tsxcount_amd -- MI355X (gfx950) k-mer counting hash map behind tsxCount's --mode=HIP.

The product is ``lib/libtsxcount_hip.so`` (hand-written HIP, C ABI in
``include/tsxcount_hip.h``).  This package is the thin host-side mirror of the
reference's ``TSXHashMap`` surface over that ABI (ctypes), used by the tests
and the bench.  There is no CPU fallback: without the built library the
first call fails, and without a GPU ``TSXHashMapHIP(...)`` raises.

Where things live (everything below is re-exported here, ``import tsxcount_amd as T`` is the surface):

_abi     the mirror of the C ABI: error codes, structures, dtypes, rule builders, the signature table, lib(), _check
models   the CPU statements of what the device computes (what the tests compare it against)
table    TSXHashMapHIP, sketch_estimate, suggest_l
group    TSXHashMapHIPGroup
textio   BGZF, wrapped FASTA, cut_records, the synth entry points, database_info
track    coverage tracks (binned k-mer counts along each sequence); reached as tsxcount_amd.track, not re-exported
correct  read correction (single substitutions undone from the spectrum); reached as tsxcount_amd.correct, not re-exported
unitig   unitigs (the compacted de Bruijn graph of a table); reached as tsxcount_amd.unitig, not re-exported
"""
import ctypes  # noqa: F401 -- ctypes, os and np stay reachable as attributes of the package (tests use T.ctypes)
import os  # noqa: F401

import numpy as np  # noqa: F401

from ._abi import (BIN_A, BIN_AMBIGUOUS, BIN_B, BIN_NAMES, BIN_NONE, BIN_STATS_DTYPE, COMBINE_COUNTS, COMBINE_OPS, EFORMAT,
                   EFULL, EHIP, EINVAL, EIO, ELOCK, ENODEVICE, ENOMEM, EOVERFLOW, EPAIR, ERANGE, HEADER_PATH, HET_MODES,
                   HET_PAIR_DTYPE, JOINT_MAX_CELLS, LIB_PATH, NO_KMER, NORMALIZE_ROUND, OK, PAIR_MODES, PREFILTER_BITS,
                   READ_MEDIAN_DTYPE, READ_STATS_DTYPE, SEQ_INTERVAL_DTYPE, SEQ_NAME_MAX, SEQ_STATS_DTYPE, SKETCH_PRECISIONS,
                   TRIM_MODES, TRIM_SPAN_DTYPE, BinIO, BinRule, BinTotals, CombineRule, CombineStats, DbInfo, FilterRule,
                   HetRule, HetStats, Layout, Level1Shape, MedianRule, NormalizeRule, NormalizeTotals, PairIO, PairTotals,
                   PrefilterTotals, SketchTotals, Stats, TrimRule, TrimTotals, TSXException, _check, _p, bin_rule, build,
                   canonical, combine_rule, decode, encode, encode_many, filter_rule, het_pair_dtype, het_rule, key_limbs, lib,
                   median_rule, min_qual_code, normalize_rule, revcomp, trim_rule)
from . import correct  # noqa: F401 -- the submodule only: its names are no part of the package's surface
from . import track  # noqa: F401 -- the submodule only: its names are no part of the package's surface
from . import unitig  # noqa: F401 -- the submodule only: its names are no part of the package's surface
from .group import TSXHashMapHIPGroup
from .models import (bin_class, fasta_records, het_histogram, het_pairs, join_fasta, joint_histogram, kmer_qv, median_count,
                     merge_sketches, missing_intervals, pair_name, prefilter_masks, sequence_stats, sketch_registers)
from .table import TSXHashMapHIP, sketch_estimate, suggest_l
from .textio import (bgzf_compress, bgzf_index, bgzf_inflate, cut_records, database_info, synth_fastq_device, synth_sizes,
                     synth_zipf_device, unwrap_fasta)
