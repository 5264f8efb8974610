"""TSXHashMapHIPGroup: one table per GPU of this node behind one object (tsx_hip_group_*)."""
import ctypes

import numpy as np

from ._abi import OK, Stats, TSXException, _check, _p, _write_counts, key_limbs, lib, min_qual_code


class TSXHashMapHIPGroup:
    """One table per GPU of this node behind one object (tsx_hip_group_*, csrc/tsx_multi.cpp): countFastq cuts the text
    into record shards, every GPU counts its own, the tables are merged (comm "rccl": RCCL, one GPU per rank; "copy":
    device copies, ranks may share a GPU), lookups go to the owner of each k-mer."""

    def __init__(self, gpus, iL, iStorageBits, iK, hash_seed=1, devices=None, comm="rccl", exchange="merge",
                 canonical=False, acgt_only=False, min_qual_char=None):
        min_qual_code(min_qual_char)
        self._lib = lib()
        self._h = ctypes.c_void_p()
        dv = (ctypes.c_int * gpus)(*devices) if devices is not None else None
        rc = self._lib.tsx_hip_group_create(ctypes.byref(self._h), gpus, dv, iK, iL, iStorageBits, 0, hash_seed,
                                            {"rccl": 0, "copy": 1}[comm])
        self._check(rc)
        self.k, self.wk, self.gpus = iK, key_limbs(iK), gpus
        if canonical:   # (the minimizer exchange refuses it)
            self._check(self._lib.tsx_hip_group_set_canonical(self._h, 1))
        self.canonical = bool(canonical)
        self._lines = 4
        self._rule = (False, None)
        if acgt_only or min_qual_char:   # (the minimizer exchange refuses it)
            self.set_base_rule(acgt_only, min_qual_char)
        if exchange != "merge":      # "mini": the minimizer exchange (20 <= k <= 32), nothing is merged afterwards
            self._check(self._lib.tsx_hip_group_set_exchange(self._h, {"merge": 0, "mini": 1}[exchange]))
        self.exchange = exchange

    @property
    def base_rule(self):
        """(acgt_only, min_qual_char) on every rank's table (see TSXHashMapHIP.set_base_rule)."""
        return self._rule

    def set_base_rule(self, acgt_only=False, min_qual_char=None):
        q = min_qual_code(min_qual_char)
        if q and self._lines != 4:
            raise ValueError("min_qual_char needs FASTQ records: a FASTA text has no quality line")
        self._check(self._lib.tsx_hip_group_set_base_rule(self._h, 1 if acgt_only else 0, q))
        self._rule = (bool(acgt_only), chr(q) if q else None)

    def _check(self, rc):
        """The group's own check: every failure carries what the group said last (tsx_hip_group_last_error)."""
        if rc != OK:
            raise TSXException(rc, self._lib.tsx_hip_strerror(rc).decode() + " (" + self._lib.tsx_hip_group_last_error().decode() + ")")

    def close(self):
        if self._h:
            self._lib.tsx_hip_group_destroy(self._h)
            self._h = ctypes.c_void_p()

    def comm_name(self):
        return self._lib.tsx_hip_group_comm_name(self._h).decode()

    def set_record_lines(self, lines):
        if lines != 4 and self._rule[1] is not None:
            raise ValueError("min_qual_char needs FASTQ records: a FASTA text has no quality line")
        self._check(self._lib.tsx_hip_group_set_record_lines(self._h, lines))
        self._lines = lines

    def clear(self):
        self._check(self._lib.tsx_hip_group_clear(self._h))

    def countFastq(self, data):
        b = bytes(data)
        self._check(self._lib.tsx_hip_group_count_fastq_host(self._h, b, len(b)))

    def getKmerCounts(self, kmers):
        k = np.ascontiguousarray(np.asarray(kmers, dtype=np.uint64).reshape(-1, self.wk))
        out = np.zeros(k.shape[0], dtype=np.uint64)
        self._check(self._lib.tsx_hip_group_get_counts_host(self._h, _p(k), k.shape[0], _p(out)))
        return out

    def stats(self):
        s = Stats()
        self._check(self._lib.tsx_hip_group_get_stats(self._h, ctypes.byref(s)))
        return s.as_dict()

    def getCountHistogram(self, nbins=10002):
        """The abundance histogram of the whole group (the sum of the ranks'; see TSXHashMapHIP.getCountHistogram)."""
        out = np.zeros(nbins, dtype=np.uint64)
        self._check(self._lib.tsx_hip_group_histogram_host(self._h, _p(out), nbins))
        return out

    def writeCounts(self, path, lower=1, upper=None, chunk_bytes=0):
        """Every k-mer of the group in [lower, upper] as "kmer<TAB>count" lines, rank after rank.  Returns (lines, bytes)."""
        return _write_counts(self._lib.tsx_hip_group_write_counts_host, self._h, self._check, path, lower, upper, chunk_bytes)

    def rank_stats(self, rank):
        s = Stats()
        _check(self._lib.tsx_hip_get_stats(self._lib.tsx_hip_group_map(self._h, rank), ctypes.byref(s)))
        return s.as_dict()

    def exchanged_entries(self):
        return int(self._lib.tsx_hip_group_exchanged_entries(self._h))

    def exchange_rounds(self):
        """Rounds of the last countFastq: pieces x shares of the minimizer exchange (TSX_HIP_MZ_PIECE / TSX_HIP_MZ_SHARE
        shrink both), 0 for the merge."""
        return int(self._lib.tsx_hip_group_exchange_rounds(self._h))
