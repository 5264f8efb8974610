"""The two helpers every file-writing and every record-fetching method of TSXHashMapHIP goes through, on the GPU.

Outputs: a method that takes a path or a caller's file descriptor writes the same bytes either way (the same lines,
for the two methods whose lines come in no particular order), leaves the caller's descriptor open, and leaves no descriptor of its own behind -- neither after the call nor after a call the library
refuses (lower > upper where the method has a range).  Open descriptors are the entries of /proc/self/fd.

Retry: queryReads, trimSpans, medianReads and binStats guess their first capacity from the text's length
(len // 256 + 16 records); a text of many short records makes the library answer ERANGE with the number needed, and
the second call must give what the device forms give in one call with ample room."""
import os

import numpy as np
import pytest

K = 15


@pytest.fixture(scope="module")
def T():
    import tsxcount_amd
    if tsxcount_amd.lib().tsx_hip_device_count() <= 0:
        pytest.fail("no GPU")
    return tsxcount_amd


def open_fds():
    return {fd: os.readlink("/proc/self/fd/" + fd) for fd in os.listdir("/proc/self/fd")
            if os.path.exists("/proc/self/fd/" + fd)}


UNORDERED = ("writeCounts", "writeHetPairs")   # their lines come "in no particular order", from one call to the next too


def written(path, unordered):
    """The bytes of a file; the sorted lines of one whose method promises no order."""
    with open(path, "rb") as f:
        data = f.read()
    return sorted(data.split(b"\n")) if unordered else data


def reads_text():
    """About 40 reads of synth.fastq, and two more that differ in one base: k-mers that pair up on their middle base."""
    from tsxcount_amd import synth
    text = synth.fastq(21, 0, 40)
    seq = text.split(b"\n")[1][:40]
    assert len(seq) == 40
    twin = seq[:15] + (b"A" if seq[15:16] != b"A" else b"C") + seq[16:]
    for name, s in ((b"het1", seq), (b"het2", twin)):
        text += b"@" + name + b"\n" + s + b"\n+\n" + b"I" * len(s) + b"\n"
    return text


def wrapped_fasta(text):
    seqs = text.split(b"\n")[1::4]
    return b"".join(b">s%d some words\n" % i + b"\n".join(s[j:j + 60] for j in range(0, len(s), 60)) + b"\n"
                    for i, s in enumerate(seqs[:12]))


def halves(text):
    lines = text.split(b"\n")[:-1]
    n = len(lines) // 8 * 4
    return b"\n".join(lines[:n]) + b"\n", b"\n".join(lines[n:2 * n]) + b"\n"


@pytest.mark.gpu
def test_path_and_descriptor_outputs(T, tmp_path):
    text = reads_text()
    fasta = wrapped_fasta(text)
    mate1, mate2 = halves(text)
    m = T.TSXHashMapHIP(18, 0, K)
    other = T.TSXHashMapHIP(17, 0, K)
    norm = T.TSXHashMapHIP(18, 0, K)
    try:
        m.countFastq(text)
        other.countFastq(mate1)
        bad = dict(lower=5, upper=4)
        # (name, number of outputs, call(outputs), the same call with arguments that are refused or None)
        cases = [
            ("writeCounts", 1, lambda o: m.writeCounts(o[0], lower=1), lambda o: m.writeCounts(o[0], **bad)),
            ("saveDatabase", 1, lambda o: m.saveDatabase(o[0]), None),
            ("writeHetPairs", 1, lambda o: m.writeHetPairs(o[0], lower=1), lambda o: m.writeHetPairs(o[0], **bad)),
            ("filterReads", 1, lambda o: m.filterReads(text, o[0], lower=1), lambda o: m.filterReads(text, o[0], **bad)),
            ("trimReads", 1, lambda o: m.trimReads(text, o[0], lower=1), lambda o: m.trimReads(text, o[0], **bad)),
            ("filterReadsByMedian", 1, lambda o: m.filterReadsByMedian(text, o[0], lower=1),
             lambda o: m.filterReadsByMedian(text, o[0], **bad)),
            ("normalizeReads", 1, lambda o: norm.normalizeReads(text, o[0]), None),   # (its refusal: below)
            ("writeSequenceStats", 1, lambda o: m.writeSequenceStats(fasta, o[0], lower=1),
             lambda o: m.writeSequenceStats(fasta, o[0], **bad)),
            ("writeMissing", 1, lambda o: m.writeMissing(fasta, o[0], lower=2), lambda o: m.writeMissing(fasta, o[0], **bad)),
            ("binReads", 4, lambda o: m.binReads(other, text, *o), lambda o: m.binReads(other, text, *o, a_range=(5, 4))),
            ("filterPairs", 4, lambda o: m.filterPairs(mate1, mate2, o[0], o[1], singles=(o[2], o[3]), lower=1),
             lambda o: m.filterPairs(mate1, mate2, o[0], o[1], singles=(o[2], o[3]), **bad)),
        ]
        for name, nout, call, refused in cases:
            # the descriptor form first: whatever the feature sets up on its first use is set up here
            by_fd = [str(tmp_path / ("%s.fd%d" % (name, i))) for i in range(nout)]
            fds = [os.open(p, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644) for p in by_fd]
            result_fd = call(fds)
            for fd in fds:
                os.fstat(fd)          # still the caller's, still open
                os.close(fd)
            by_path = [str(tmp_path / ("%s.path%d" % (name, i))) for i in range(nout)]
            before = open_fds()
            result_path = call(by_path)
            assert open_fds() == before, name
            assert result_path == result_fd, name
            got = [written(p, name in UNORDERED) for p in by_path]
            assert got == [written(p, name in UNORDERED) for p in by_fd], name
            assert sum(len(g) for g in got) > 0, name + ": nothing written, nothing compared"
            if refused is not None:
                with pytest.raises((T.TSXException, ValueError)):
                    refused([str(tmp_path / ("%s.refused%d" % (name, i))) for i in range(nout)])
                assert open_fds() == before, name + " (refused)"
        assert m.writeHetPairs(str(tmp_path / "het"), lower=1)[0] >= 1
        # normalizeReads has no range; it refuses a map whose prefilter is armed, after the output has been opened
        norm.createPrefilter(12)
        norm.armPrefilter(True)
        before = open_fds()
        with pytest.raises(T.TSXException) as e:
            norm.normalizeReads(text, str(tmp_path / "normalize.refused"))
        assert e.value.code == T.EINVAL and "prefilter is armed" in str(e.value)
        assert open_fds() == before
        # addDatabase reads: both forms load the same table, and a file that is no database is closed again
        db = str(tmp_path / "saveDatabase.path0")
        loaded = []
        for form in ("fd", "path"):
            fresh = T.TSXHashMapHIP(18, 0, K)
            try:
                if form == "fd":
                    fd = os.open(db, os.O_RDONLY)
                    n = fresh.addDatabase(fd)
                    os.fstat(fd)
                    os.close(fd)
                else:
                    before = open_fds()
                    n = fresh.addDatabase(db)
                    assert open_fds() == before
                kmers, counts = fresh.getAllKmers()
                loaded.append((n, sorted(zip(kmers[:, 0].tolist(), counts.tolist()))))
                before = open_fds()
                with pytest.raises(T.TSXException):
                    fresh.addDatabase(str(tmp_path / "filterReads.path0"))
                assert open_fds() == before, form + " (refused)"
            finally:
                fresh.close()
        assert loaded[0] == loaded[1] and loaded[0][0] > 0 and len(loaded[0][1]) == m.stats()["distinct"]
    finally:
        m.close()
        other.close()
        norm.close()


def short_records(n=200, length=20, pool=50, seed=7):
    """n two-line FASTA records of `length` bases drawn from `pool` distinct sequences: about 27 bytes a record, so the
    first capacity of a text of them (bytes // 256 + 16) is far below n."""
    rng = np.random.RandomState(seed)
    seqs = [bytes(rng.choice(list(b"ACGT"), length).astype(np.uint8)) for _ in range(pool)]
    return b"".join(b">r%03d\n" % i + seqs[rng.randint(pool)] + b"\n" for i in range(n))


@pytest.mark.gpu
def test_record_arrays_after_the_second_call(T):
    import torch
    n = 200
    text = short_records(n)
    assert len(text) // 256 + 16 < n // 4            # the first call cannot hold them
    a = T.TSXHashMapHIP(16, 0, K)
    b = T.TSXHashMapHIP(17, 0, K)
    try:
        for m, counted in ((a, text), (b, text[:len(text) // 2])):
            m.set_record_lines(2)
            m.countFastq(counted)
        dev = torch.zeros(len(text) + 64, dtype=torch.uint8, device="cuda:0")
        dev[:len(text)] = torch.frombuffer(bytearray(text), dtype=torch.uint8).to("cuda:0")
        cap = n + 56

        def device_form(dtype, call):
            buf = torch.zeros((cap, dtype.itemsize // 8), dtype=torch.int64, device="cuda:0")
            assert call(buf.data_ptr()) == n
            return buf.cpu().numpy().view(np.uint64).reshape(-1).view(dtype)[:n]

        got = a.queryReads(text, lower=2)
        want = device_form(T.READ_STATS_DTYPE, lambda p: a.queryReadsDevice(dev.data_ptr(), len(text), p, cap, lower=2))
        assert got.dtype == T.READ_STATS_DTYPE and len(got) == n and np.array_equal(got, want)
        assert (got["kmers"] == 20 - K + 1).all() and got["in_range"].max() > 0

        got = a.trimSpans(text, lower=2)
        rule = T.trim_rule(2, None, "longest")
        want = device_form(T.TRIM_SPAN_DTYPE, lambda p: a.trimSpansDevice(dev.data_ptr(), len(text), p, cap, rule))
        assert got.dtype == T.TRIM_SPAN_DTYPE and len(got) == n and np.array_equal(got, want)
        assert got["length"].max() == 20

        got = a.medianReads(text)
        want = device_form(T.READ_MEDIAN_DTYPE, lambda p: a.medianReadsDevice(dev.data_ptr(), len(text), p, cap))
        assert got.dtype == T.READ_MEDIAN_DTYPE and len(got) == n and np.array_equal(got, want)
        assert got["median"].min() >= 1 and got["median"].max() > 1

        got, classes = a.binStats(b, text)
        want = device_form(T.BIN_STATS_DTYPE, lambda p: a.binStatsDevice(b, dev.data_ptr(), len(text), p, cap))
        assert got.dtype == T.BIN_STATS_DTYPE and len(got) == n and np.array_equal(got, want)
        assert classes.dtype == np.uint8 and len(classes) == n
        assert classes.tolist() == [T.bin_class(r["hits_a"], r["hits_b"]) for r in got]
        assert len(set(classes.tolist())) > 1
    finally:
        a.close()
        b.close()
