"""Coverage tracks: the k-mer counts of the sequences of a wrapped FASTA in bins of `window` start positions
(csrc/tsx_track.h, tsx_hip_seq_track_*).  A submodule of its own: the functions take the map, ``track.sequence_track(m, text,
1000)``; nothing here is re-exported by the package.

A sequence of length L has ceil(L / window) bins; bin b covers the start positions [b * window, min((b + 1) * window, L)) of
the joined sequence and holds (SEQ_BIN_DTYPE) kmers, present, min_count, max_count, sum_count over the windows that
start there.  The device calls return (names, stats, first, bins): names and stats as querySequences, bins of sequence i
= bins[first[i]:first[i + 1]].  track_bins states the same on the CPU; format_track is the text of write_sequence_track.
"""
import ctypes

import numpy as np

from ._abi import _check, _fds, _stream, _upper, lib
from .models import _seq_table, _seq_window_counts

SEQ_BIN_DTYPE = np.dtype([("kmers", np.uint64), ("present", np.uint64), ("min_count", np.uint64), ("max_count", np.uint64),
                          ("sum_count", np.uint64)])
WINDOW_MIN, WINDOW_MAX = 64, 1 << 32


def _track_of(m, res):
    """(names, stats, first, bins) of a result with a track."""
    names, stats = m._seq_stats_of(res)
    bins_p, first_p = ctypes.c_void_p(None), ctypes.c_void_p(None)
    n = lib().tsx_hip_seq_result_bins(res, ctypes.byref(bins_p), ctypes.byref(first_p))
    first = np.zeros(len(names) + 1, dtype=np.uint64)
    ctypes.memmove(first.ctypes.data, first_p.value, first.nbytes)
    bins = np.zeros(n, dtype=SEQ_BIN_DTYPE)
    if n:
        ctypes.memmove(bins.ctypes.data, bins_p.value, bins.nbytes)
    return names, stats, first, bins


def sequence_track(m, text, window, lower=1, upper=None, chunk_bytes=0):
    """The track of a wrapped FASTA text in host memory against the table m (tsx_hip_seq_track_host): (names, stats,
    first, bins); what track_bins states on the CPU.  TSXException EINVAL for what querySequences refuses and for a
    window outside 64 .. 2^32."""
    b = bytes(text)

    def call(handle, *a):
        return lib().tsx_hip_seq_track_host(handle, b, len(b), int(lower), _upper(upper), int(window), int(chunk_bytes), *a)
    return m._seq_call(call, (), lambda res: _track_of(m, res))


def sequence_track_bgzf(m, gz, window, lower=1, upper=None):
    """sequence_track for the image of a blocked gzip (BGZF) file."""
    b = bytes(gz)

    def call(handle, *a):
        return lib().tsx_hip_seq_track_bgzf_host(handle, b, len(b), int(lower), _upper(upper), int(window), *a)
    return m._seq_call(call, (), lambda res: _track_of(m, res))


def sequence_track_device(m, text_ptr, nbytes, window, lower=1, upper=None, stream=None):
    """sequence_track for a wrapped FASTA text resident on the device (16-byte aligned)."""
    def call(handle, *a):
        return lib().tsx_hip_seq_track_device(handle, ctypes.c_void_p(text_ptr), nbytes, int(lower), _upper(upper), int(window),
                                              *a, _stream(stream))
    return m._seq_call(call, (), lambda res: _track_of(m, res))


def write_sequence_track(m, text, path_or_fd, window, lower=1, upper=None, chunk_bytes=0):
    """One line per bin to a path or an open file descriptor: name, start, end, kmers, present, min, max, mean
    (tsx_hip_seq_write_track).  Returns the number of bins."""
    b = bytes(text)

    def call(handle, *a):
        return lib().tsx_hip_seq_track_host(handle, b, len(b), int(lower), _upper(upper), int(window), int(chunk_bytes), *a)
    with _fds(path_or_fd) as (fd,):
        def use(res):
            _check(lib().tsx_hip_seq_write_track(res, fd), refusal=True)
            return int(lib().tsx_hip_seq_result_bins(res, None, None))
        return m._seq_call(call, (), use)


def track_bins(records, counts, k, window, lower=1, upper=None, canonical=False, acgt_only=False):
    """(first, bins) of the records of fasta_records against counts ({k-mer bytes: count}), with the conventions of
    sequence_stats: bins is a list of (kmers, present, min_count, max_count, sum_count), one per bin of every record in
    order, first the len(records) + 1 offsets into it.  A record of length L has ceil(L / window) bins; a window belongs to
    the bin of its start position; windows the base rule drops are no k-mers; min and max are 0 without k-mers, the sum
    is taken modulo 2^64."""
    window = int(window)
    if not WINDOW_MIN <= window <= WINDOW_MAX:
        raise ValueError("track window %d outside 64 .. 2^32" % window)
    upper = _upper(upper)
    tab = _seq_table(counts, canonical)
    first, bins = [0], []
    for _, seq in records:
        cs = _seq_window_counts(seq, tab, k, canonical, acgt_only)
        for a in range(0, len(seq), window):
            c = [x for x in cs[a:a + window] if x is not None]
            bins.append((len(c), sum(lower <= x <= upper for x in c), min(c) if c else 0, max(c) if c else 0, sum(c) % (1 << 64)))
        first.append(len(bins))
    return first, bins


def format_track(names, first, bins, window, lengths):
    """The bytes tsx_hip_seq_write_track writes: per bin name, start, end, kmers, present, min, max, mean, tab-separated;
    the mean is sum / kmers as %.4f, NA without k-mers; an empty name is written *.  bins: rows of (kmers, present,
    min_count, max_count, sum_count); lengths: the length of every sequence (the end of its last bin)."""
    out = []
    for i, name in enumerate(names):
        for b, at in enumerate(range(int(first[i]), int(first[i + 1]))):
            kmers, present, mn, mx, total = (int(v) for v in bins[at])
            mean = b"%.4f" % (float(total) / float(kmers)) if kmers else b"NA"
            out.append(b"%s\t%d\t%d\t%d\t%d\t%d\t%d\t%s\n" % (bytes(name) or b"*", b * window, min((b + 1) * window, int(lengths[i])),
                                                              kmers, present, mn, mx, mean))
    return b"".join(out)
