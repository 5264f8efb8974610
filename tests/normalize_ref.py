"""Digital normalization in plain Python: the definition that tests/test_normalize.py compares the library with.

Records are numbered from 0 over the whole text; round j holds the records [j R, (j + 1) R).  For each round in order
every record gets its median against the Counter as it stands (saturated counts, sorted(values)[m // 2], 0 for a
record without k-mers); a record is kept iff median < cutoff; after the whole round is judged every k-mer occurrence
of its kept records is added.  The window rule is test_trim.solid_flags, the records are those of
test_read_query.records.  Never the library under test."""
from collections import Counter

from test_median_cpu import SAT
from test_read_query import _CODE, U64, line_spans, rc
from test_trim import solid_flags


def record_kmers(text, k, lpr, canonical=False, acgt_only=False, minq=0):
    """Per record: (the keys of its k-mers in order -- coded, folded when canonical -- and its bytes as written)."""
    sp = line_spans(text)
    out = []
    for i in range(0, len(sp), lpr):
        grp = sp[i:i + lpr]
        seq = text[grp[1][0]:grp[1][1]] if len(grp) > 1 else b""
        qual = text[grp[3][0]:grp[3][1]] if len(grp) > 3 else b""
        is_kmer = solid_flags(seq, qual, {}, k, 0, U64, canonical, acgt_only, minq)
        s = seq.translate(_CODE)
        keys = []
        for j, ok in enumerate(is_kmer):
            if ok:
                x = s[j:j + k]
                keys.append(min(x, rc(x)) if canonical else x)
        out.append((keys, text[grp[0][0]:grp[-1][1]] + b"\n"))
    return out


def normalize(text, k, lpr, cutoff, R, counts=None, **rule):
    """(keep flags, output bytes, totals dict, Counter).  `counts`: the table at the start (not modified)."""
    assert R >= 1
    table = Counter(counts or {})
    recs = record_kmers(text, k, lpr, **rule)
    keep = []
    tot = {"records": len(recs), "kept": 0, "kmers_seen": 0, "kmers_added": 0, "rounds": (len(recs) + R - 1) // R}
    for r0 in range(0, len(recs), R):
        rnd = recs[r0:r0 + R]
        verdict = []
        for keys, _ in rnd:
            vals = sorted(min(table[x], SAT) for x in keys)
            verdict.append((vals[len(vals) // 2] if vals else 0) < cutoff)
        for (keys, _), kp in zip(rnd, verdict):
            tot["kmers_seen"] += len(keys)
            if kp:
                tot["kept"] += 1
                tot["kmers_added"] += len(keys)
                table.update(keys)
        keep += verdict
    table = Counter({x: c for x, c in table.items() if c})
    return keep, b"".join(r for (_, r), kp in zip(recs, keep) if kp), tot, table
