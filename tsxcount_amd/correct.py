"""Read correction: single substitutions undone from the k-mer spectrum (csrc/tsx_correct.h, tsx_hip_correct_*).  A
submodule of its own: the functions take the map, ``correct.correct_reads(m, text)``; nothing here is re-exported by the
package.

The rule (include/tsxcount_hip.h states it in full): a window of a sequence line is solid when it is a k-mer under the
table's base rule and its count lies in lower..upper.  A maximal run [a, b] of non-solid windows is a site when it is what
ONE wrong base leaves behind -- k windows inside the read, at most k at either end -- and its suspect base p is the one
base all its windows share.  The three other bases are tried at p; when exactly one of them makes every window a..b
solid, the byte is replaced (in the case it had).  Sites never share a window, so each is judged on the original text.
correct_model states the same on the CPU, from the text and a dict of counts alone.
"""
import ctypes
import tempfile

import numpy as np

from ._abi import ERANGE, CorrectRule, CorrectTotals, _check, _fds, _stream, _upper, lib
from .models import _ACGT, _seq_table, _seq_window_counts

CORRECTION_DTYPE = np.dtype([("record", np.uint64), ("pos", np.uint32), ("from", np.uint8), ("to", np.uint8),
                             ("windows", np.uint16)])


def correct_rule(lower=2, upper=None, min_windows=1):
    """A CorrectRule from the Python arguments.  Raises ValueError for lower > upper, before any GPU call."""
    upper = _upper(upper)
    if int(lower) > upper:
        raise ValueError("correct range: lower %d > upper %d" % (int(lower), upper))
    return CorrectRule(int(lower), upper, int(min_windows), 0)


def correction_sites(m, text, lower=2, upper=None, min_windows=1, chunk_bytes=0, cap=None):
    """The corrections of a FASTQ / FASTA text in host memory against the table m (tsx_hip_correct_sites_host):
    (a numpy structured array CORRECTION_DTYPE sorted by (record, pos), the totals as a dict).  cap: room for that
    many corrections only -- more of them raise TSXException ERANGE; None: as many as there are."""
    rule = correct_rule(lower, upper, min_windows)
    b = bytes(text)
    tot, n = CorrectTotals(), ctypes.c_size_t(0)
    room = len(b) // 256 + 16 if cap is None else int(cap)
    for _ in range(2):
        out = np.zeros(room, dtype=CORRECTION_DTYPE)
        rc = lib().tsx_hip_correct_sites_host(m.handle, b, len(b), ctypes.byref(rule), out.ctypes.data_as(ctypes.c_void_p), room,
                                              ctypes.byref(n), ctypes.byref(tot), int(chunk_bytes))
        if rc != ERANGE or cap is not None:
            break
        room = n.value
    _check(rc, refusal=True)
    return out[:n.value], tot.as_dict()


def correct_reads(m, text, path_or_fd=None, lower=2, upper=None, min_windows=1, chunk_bytes=0):
    """The text with its corrections applied (tsx_hip_correct_reads_host), written to a path (created or truncated) or an
    open file descriptor; returns the totals as a dict.  Without an output the corrected bytes are returned in front of
    them: (bytes, totals).  The output has the input's length."""
    rule = correct_rule(lower, upper, min_windows)
    b = bytes(text)
    tot = CorrectTotals()

    def call(fd):
        _check(lib().tsx_hip_correct_reads_host(m.handle, b, len(b), ctypes.byref(rule), fd, int(chunk_bytes), ctypes.byref(tot)),
               refusal=True)
    if path_or_fd is None:
        with tempfile.TemporaryFile() as f:
            call(f.fileno())
            f.seek(0)
            return f.read(), tot.as_dict()
    with _fds(path_or_fd) as (fd,):
        call(fd)
    return tot.as_dict()


def correction_sites_device(m, text_ptr, nbytes, corrections_ptr, cap, lower=2, upper=None, min_windows=1, stream=None):
    """tsx_hip_correct_sites_device: the corrections of a device text (16-byte aligned) into a device buffer of cap
    records, in no order.  Returns (their number, totals); more than cap: TSXException ERANGE."""
    rule = correct_rule(lower, upper, min_windows)
    tot, n = CorrectTotals(), ctypes.c_size_t(0)
    _check(lib().tsx_hip_correct_sites_device(m.handle, ctypes.c_void_p(text_ptr), nbytes, ctypes.byref(rule),
                                              ctypes.c_void_p(corrections_ptr), cap, ctypes.byref(n), ctypes.byref(tot),
                                              _stream(stream)), refusal=True)
    return int(n.value), tot.as_dict()


def correct_reads_device(m, text_ptr, nbytes, out_ptr, lower=2, upper=None, min_windows=1, stream=None):
    """tsx_hip_correct_reads_device: the nbytes of a device text with the corrections applied into out_ptr (nbytes of
    room; may be text_ptr).  Returns the totals."""
    rule = correct_rule(lower, upper, min_windows)
    tot = CorrectTotals()
    _check(lib().tsx_hip_correct_reads_device(m.handle, ctypes.c_void_p(text_ptr), nbytes, ctypes.byref(rule),
                                              ctypes.c_void_p(out_ptr), nbytes, ctypes.byref(tot), _stream(stream)), refusal=True)
    return tot.as_dict()


def _lines(text):
    """(start, end) of every non-empty line, split at b"\\n" (b"\\r" is an ordinary byte)."""
    out, pos = [], 0
    for part in text.split(b"\n"):
        if part:
            out.append((pos, pos + len(part)))
        pos += len(part) + 1
    return out


def correct_model(text, counts, k, lower=2, upper=None, min_windows=1, canonical=False, acgt_only=False, lines_per_record=4):
    """The rule on the CPU: (corrected bytes, [(record, pos, from, to, windows)] sorted, totals) of a text against counts
    ({k-mer bytes: count}, keys as sequence_stats takes them).  Records are the non-empty lines in groups of
    lines_per_record, the sequence is the second line of a group, as for the trim.  Which windows are k-mers and what
    they count -- every byte folded through base_code (an N reads as A), acgt_only dropping windows with another byte --
    is NOT stated a second time here: it is _seq_window_counts of models.py, shared with sequence_stats, so a change
    there changes this model too."""
    upper = _upper(upper)
    text = bytes(text)
    tab = _seq_table(counts, canonical)
    out, fixes = bytearray(text), []
    tot = dict(records=0, sites=0, corrected=0, ambiguous=0, unfixable=0, bytes=len(text))
    sp = _lines(text)

    def solid(seq):
        return [c is not None and lower <= c <= upper for c in _seq_window_counts(seq, tab, k, canonical, acgt_only)]

    for r, g in enumerate(range(0, len(sp), lines_per_record)):
        tot["records"] += 1
        grp = sp[g:g + lines_per_record]
        if len(grp) < 2:
            continue
        s0, seq = grp[1][0], text[grp[1][0]:grp[1][1]]
        n = len(seq) - k + 1
        if n < 2:
            continue
        ok, a = solid(seq), 0
        while a < n:
            if ok[a]:
                a += 1
                continue
            b = a
            while b + 1 < n and not ok[b + 1]:
                b += 1
            w, head, tail = b - a + 1, a == 0, b == n - 1
            site = w >= min_windows and not (head and tail) and (w == k if not (head or tail) else w <= k)
            if site:
                p = a + k - 1 if tail else b
                tot["sites"] += 1
                good = []
                if seq[p] in _ACGT:
                    c = b"ACGT".index(bytes([seq[p] & 0xDF]))
                    for d in (1, 2, 3):
                        alt = seq[:p] + bytes([b"ACGT"[c ^ d] | (seq[p] & 0x20)]) + seq[p + 1:]
                        if all(solid(alt[a:b + k])):
                            good.append(alt[p])
                if len(good) == 1:
                    tot["corrected"] += 1
                    fixes.append((r, p, seq[p], good[0], w))
                    out[s0 + p] = good[0]
                elif good:
                    tot["ambiguous"] += 1
                else:
                    tot["unfixable"] += 1
            a = b + 1
    return bytes(out), fixes, tot
