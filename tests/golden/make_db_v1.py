#!/usr/bin/env python3
"""Regenerates tests/golden/small_t7.first8.k14.v1.db (needs a GPU): the first 8 records of small_t7.1000.fastq counted
at k=14, l=10, s=2 (2-bit counters, so that the file holds carry records), hash seed 1234, saved as a version-1 k-mer
database in 256-slot chunks.  test_database_format.py loads it as a file written by an earlier build: a change of the
format that breaks old files fails there.  Run it only when the format version changes, and keep the old file."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

FASTQ = os.path.join(HERE, "small_t7.1000.fastq")
OUT = os.path.join(HERE, "small_t7.first8.k14.v1.db")
K, L, S, SEED, RECORDS = 14, 10, 2, 1234, 8


def first_records(n=RECORDS):
    with open(FASTQ, "rb") as f:
        lines = f.read().split(b"\n")
    return b"\n".join(lines[:4 * n]) + b"\n"


def main(out=OUT):
    import torch
    torch.zeros(1, device="cuda:0")   # the runtime torch brings, first (tests/conftest.py says why)
    import tsxcount_amd as T
    m = T.TSXHashMapHIP(L, S, K, hash_seed=SEED)
    m.countFastq(first_records())
    assert m.stats()["overflow_used"] > 0, m.stats()
    entries, nbytes = m.saveDatabase(out, chunk_bytes=32 + 256 // 64 * 8 + 256 * 8)
    print("%s: %d entries, %d bytes, %s" % (out, entries, nbytes, m.stats()))
    m.close()


if __name__ == "__main__":
    main(*sys.argv[1:])
