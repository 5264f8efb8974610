"""Unitigs: the compacted de Bruijn graph of a k-mer table (csrc/tsx_unitig.h, tsx_hip_unitig*).  A submodule of its own:
the functions take the map, ``unitig.unitigs(m)``; nothing here is re-exported by the package.

The definitions (include/tsxcount_hip.h and DESIGN.md §3 "Unitigs" state them in full).  The nodes are the k-mers whose
count lies in lower..upper; on a canonical table a node stands for both strands.  An oriented node is a node read as a
string s.  succ(s) are the strings s[1:] + c that are nodes, pred(s) the strings c + s[:-1] that are.  An edge s -> t, t in
succ(s), is compactable when |succ(s)| = 1, |pred(t)| = 1 and t is not the node of s.  A unitig is a maximal chain of
compactable edges, spelled as its first string and the last base of every later one; on a canonical table the smaller of
the spelling and its reverse complement is reported (k is odd there).  A chain that closes on itself is cut at a node of
the implementation's choice and marked circular.  unitig_model states the same on the CPU from a dict of counts alone;
check_unitigs checks a result against the definitions without calling the model.
"""
import ctypes

import numpy as np

from ._abi import ERANGE, UnitigRule, UnitigTotals, _check, _fds, _stream, _upper, lib

UNITIG_DTYPE = np.dtype([("offset", np.uint64), ("length", np.uint64), ("kmers", np.uint64), ("sum_count", np.uint64),
                         ("circular", np.uint64)])

_COMP = bytes.maketrans(b"ACGT", b"TGCA")
_BASES = (b"A", b"C", b"G", b"T")


def _rc(s):
    return s[::-1].translate(_COMP)


def unitig_rule(lower=1, upper=None):
    """A UnitigRule from the Python arguments.  Raises ValueError for lower > upper, before any GPU call."""
    upper = _upper(upper)
    if int(lower) > upper:
        raise ValueError("unitigs: lower %d > upper %d" % (int(lower), upper))
    return UnitigRule(int(lower), upper, 0, 0)


def unitig_stats(m, lower=1, upper=None):
    """The totals of the unitigs of the table m (tsx_hip_unitig_stats): the degree sweep and the walks, nothing spelled."""
    rule = unitig_rule(lower, upper)
    tot = UnitigTotals()
    _check(lib().tsx_hip_unitig_stats(m.handle, ctypes.byref(rule), ctypes.byref(tot)), refusal=True)
    return tot.as_dict()


def unitigs(m, lower=1, upper=None):
    """The unitigs of the table m in host memory (tsx_hip_unitigs_host): (the bytes of all sequences, a numpy structured
    array UNITIG_DTYPE, the totals as a dict); the sequence of record r is seq[r.offset:r.offset + r.length].  The order
    of the records is unspecified.  The first call guesses the room; on ERANGE the call is made once more with the
    sizes the library reported."""
    rule = unitig_rule(lower, upper)
    tot, n, nbytes = UnitigTotals(), ctypes.c_size_t(0), ctypes.c_size_t(0)
    rec_cap, seq_cap = 1 << 12, 1 << 18
    for _ in range(2):
        seq = np.zeros(max(seq_cap, 1), dtype=np.uint8)
        rec = np.zeros(max(rec_cap, 1), dtype=UNITIG_DTYPE)
        rc = lib().tsx_hip_unitigs_host(m.handle, ctypes.byref(rule), seq.ctypes.data_as(ctypes.c_void_p), seq_cap,
                                        rec.ctypes.data_as(ctypes.c_void_p), rec_cap, ctypes.byref(n), ctypes.byref(nbytes),
                                        ctypes.byref(tot))
        if rc != ERANGE:
            break
        rec_cap, seq_cap = n.value, nbytes.value
    _check(rc, refusal=True)
    return seq[:nbytes.value].tobytes(), rec[:n.value], tot.as_dict()


def unitig_strings(seq, records):
    """The sequence of every record as bytes, in the records' order."""
    seq = bytes(seq)
    return [seq[int(r["offset"]):int(r["offset"]) + int(r["length"])] for r in records]


def unitigs_device(m, seq_ptr, seq_cap, rec_ptr, rec_cap, lower=1, upper=None, stream=None):
    """tsx_hip_unitigs_device: sequences and records (UNITIG_DTYPE) into device buffers of seq_cap bytes and rec_cap
    records.  Returns (records, sequence bytes, totals).  A buffer too small: TSXException ERANGE, whose `needed`
    attribute holds (records, sequence bytes) and nothing is spelled."""
    rule = unitig_rule(lower, upper)
    tot, n, nbytes = UnitigTotals(), ctypes.c_size_t(0), ctypes.c_size_t(0)
    rc = lib().tsx_hip_unitigs_device(m.handle, ctypes.byref(rule), ctypes.c_void_p(seq_ptr), int(seq_cap),
                                      ctypes.c_void_p(rec_ptr), int(rec_cap), ctypes.byref(n), ctypes.byref(nbytes),
                                      ctypes.byref(tot), _stream(stream))
    try:
        _check(rc, refusal=True)
    except Exception as e:  # noqa: BLE001 -- the sizes travel with the ERANGE
        e.needed = (int(n.value), int(nbytes.value))
        raise
    return int(n.value), int(nbytes.value), tot.as_dict()


def write_unitigs(m, path_or_fd, lower=1, upper=None):
    """The unitigs as FASTA to a path (created or truncated) or an open file descriptor (tsx_hip_write_unitigs_host):
    `>INDEX LN:i:<bases> KC:i:<sum_count> km:f:<sum_count / kmers>`, ` CL:i:1` behind it for a circular one, the
    sequence on one line.  Returns the totals as a dict."""
    rule = unitig_rule(lower, upper)
    tot = UnitigTotals()
    with _fds(path_or_fd) as (fd,):
        _check(lib().tsx_hip_write_unitigs_host(m.handle, ctypes.byref(rule), fd, ctypes.byref(tot)), refusal=True)
    return tot.as_dict()


def format_unitigs(unitigs):
    """The bytes write_unitigs writes for unitigs (sequence, kmers, sum_count, circular) in the given order."""
    out = []
    for i, (seq, kmers, total, circular) in enumerate(unitigs):
        out.append(b">%d LN:i:%d KC:i:%d km:f:%.1f%s\n%s\n" % (i, len(seq), total, float(total) / float(kmers),
                                                              b" CL:i:1" if circular else b"", bytes(seq)))
    return b"".join(out)


def _nodes(counts, k, lower, upper, canonical):
    """{node: count} of the k-mers in range; on a canonical table keyed by the smaller strand, the strands' counts summed."""
    if canonical and k % 2 == 0:
        raise ValueError("unitigs: even k on a canonical table")
    upper = _upper(upper)
    if int(lower) > upper:
        raise ValueError("unitigs: lower %d > upper %d" % (int(lower), upper))
    tab = {}
    for s, c in counts.items():
        s = bytes(s)
        if len(s) != k:
            raise ValueError("unitigs: %r is no %d-mer" % (s, k))
        key = min(s, _rc(s)) if canonical else s
        tab[key] = tab.get(key, 0) + int(c)
    return {s: c for s, c in tab.items() if c >= 1 and int(lower) <= c <= upper}


def unitig_model(counts, k, lower=1, upper=None, canonical=False):
    """The definition on the CPU over counts ({k-mer bytes: count}): (a list of (sequence, kmers, sum_count, circular),
    the totals as unitig_stats gives them).  Strings and sets, no hashing.  A cycle is cut at its smallest node, read as
    that node's smaller strand."""
    nodes = _nodes(counts, k, lower, upper, canonical)

    def node(s):
        return min(s, _rc(s)) if canonical else s

    def succ(s):
        return [s[1:] + c for c in _BASES if node(s[1:] + c) in nodes]

    def pred(s):
        return [c + s[:-1] for c in _BASES if node(c + s[:-1]) in nodes]

    def follow(s):
        """The t of the compactable edge s -> t, or None."""
        out = succ(s)
        if len(out) != 1 or len(pred(out[0])) != 1 or node(out[0]) == node(s):
            return None
        return out[0]

    def before(s):
        """The p of the compactable edge p -> s, or None."""
        inn = pred(s)
        if len(inn) != 1 or len(succ(inn[0])) != 1 or node(inn[0]) == node(s):
            return None
        return inn[0]

    def chain(s, stop=None):
        path = [s]
        while True:
            t = follow(path[-1])
            if t is None or t == stop:
                return path
            if len(path) > len(nodes):
                raise RuntimeError("unitigs: a chain longer than the graph")
            path.append(t)

    def spell(path):
        return path[0] + b"".join(s[-1:] for s in path[1:])

    out, seen = [], set()
    for v in sorted(nodes):
        for s in ((v, _rc(v)) if canonical else (v,)):
            if node(s) in seen or before(s) is not None:
                continue
            path = chain(s)
            seq = spell(path)
            if canonical:
                seq = min(seq, _rc(seq))
            seen.update(node(x) for x in path)
            out.append((seq, len(path), sum(nodes[node(x)] for x in path), False))
    for v in sorted(nodes):
        if v in seen:
            continue
        path = chain(v, stop=v)
        seen.update(node(x) for x in path)
        out.append((spell(path), len(path), sum(nodes[node(x)] for x in path), True))

    deg = [0] * 25
    tot = dict(nodes=len(nodes), unitigs=len(out), circular=sum(1 for u in out if u[3]), bases=sum(len(u[0]) for u in out),
               longest=max([len(u[0]) for u in out] or [0]), isolated=0, tips=0, branching=0, sum_count=sum(nodes.values()))
    for v in nodes:   # the degrees of a node are those of the strand a dump reports
        i, o = len(pred(v)), len(succ(v))
        deg[i * 5 + o] += 1
        tot["isolated"] += i == 0 and o == 0
        tot["tips"] += (i == 0) != (o == 0)
        tot["branching"] += i > 1 or o > 1
    tot["degree"] = deg
    return out, tot


def check_unitigs(unitigs, counts, k, lower=1, upper=None, canonical=False):
    """An independent check of unitigs -- (sequence, kmers, sum_count, circular) each -- against the definitions, from
    counts alone and without unitig_model.  Raises AssertionError with what is wrong: a k-mer in range missing or there
    twice (either strand on canonical), a k-mer that is no node, an inner junction that is no compactable edge, an end that
    a compactable edge extends, kmers or sum_count wrong, on a canonical table a sequence greater than its reverse
    complement, a circular one that does not close."""
    if canonical and k % 2 == 0:
        raise ValueError("unitigs: even k on a canonical table")
    key = (lambda s: min(s, _rc(s))) if canonical else (lambda s: s)
    hi = (1 << 64) - 1 if upper is None else int(upper)
    folded = {}                     # the node set, made here a second time: nothing is shared with the model
    for s, c in counts.items():
        folded[key(bytes(s))] = folded.get(key(bytes(s)), 0) + int(c)
    nodes = {s: c for s, c in folded.items() if len(s) == k and c > 0 and int(lower) <= c <= hi}
    present = lambda s: key(s) in nodes   # noqa: E731
    outs = lambda s: [s[1:] + c for c in _BASES if present(s[1:] + c)]   # noqa: E731
    ins = lambda s: [c + s[:-1] for c in _BASES if present(c + s[:-1])]   # noqa: E731

    def compactable(s, t):
        return outs(s) == [t] and ins(t) == [s] and key(s) != key(t)

    seen = {}
    for n, (seq, kmers, total, circular) in enumerate(unitigs):
        seq = bytes(seq)
        assert len(seq) >= k, "unitig %d: shorter than k" % n
        win = [seq[i:i + k] for i in range(len(seq) - k + 1)]
        assert int(kmers) == len(win), "unitig %d: kmers %d, the sequence holds %d" % (n, kmers, len(win))
        for s in win:
            assert present(s), "unitig %d: %r is no node" % (n, s)
            assert key(s) not in seen, "%r lies in unitigs %d and %d" % (s, seen[key(s)], n)
            seen[key(s)] = n
        assert int(total) == sum(nodes[key(s)] for s in win), "unitig %d: sum_count %d" % (n, total)
        for s, t in zip(win, win[1:]):
            assert compactable(s, t), "unitig %d: %r -> %r is no compactable edge" % (n, s, t)
        if circular:
            assert compactable(win[-1], win[0]) and win[-1][1:] + win[0][-1:] == win[0], "unitig %d: does not close" % n
        else:
            assert not any(compactable(p, win[0]) for p in ins(win[0])), "unitig %d: extends to the left" % n
            assert not any(compactable(win[-1], t) for t in outs(win[-1])), "unitig %d: extends to the right" % n
            if canonical:
                assert seq <= _rc(seq), "unitig %d: the greater strand" % n
    missing = [s for s in nodes if s not in seen]
    assert not missing, "%d nodes in no unitig, e.g. %r" % (len(missing), missing[0])
