"""Free helpers around the inputs and files of a count: BGZF images, wrapped FASTA, record cuts, the synthetic reads
made on the device, and the header of a k-mer database file."""
import ctypes

import numpy as np

from ._abi import EINVAL, OK, DbInfo, TSXException, _check, _fds, _p, _stream, lib


def bgzf_index(gz):
    """(members, text bytes) of a BGZF image, or None when the buffer is not BGZF."""
    b = bytes(gz)
    nm, nb = ctypes.c_size_t(0), ctypes.c_size_t(0)
    rc = lib().tsx_hip_bgzf_index_host(b, len(b), ctypes.byref(nm), ctypes.byref(nb))
    return (nm.value, nb.value) if rc == OK else None


def bgzf_inflate(gz, device=0):
    """Inflate a BGZF image on the device and return the text (tests, tools)."""
    b = bytes(gz)
    ix = bgzf_index(b)
    if ix is None:
        raise TSXException(EINVAL, "not a BGZF image")
    out = ctypes.create_string_buffer(max(ix[1], 1))
    got = ctypes.c_size_t(0)
    _check(lib().tsx_hip_inflate_bgzf_host(device, b, len(b), out, ix[1], ctypes.byref(got)), refusal=True)
    return out.raw[:got.value]


def bgzf_compress(data, level=6, block=65280):
    """BGZF writer (the layout `bgzip` produces: SAM specification section 4.1) -- for tests and tools; zlib does
    the deflate, one gzip member with a BC extra field per `block` bytes, the empty end-of-file member last."""
    import struct
    import zlib
    out = bytearray()
    data = bytes(data)
    for i in range(0, len(data), block):
        chunk = data[i:i + block]
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        raw = c.compress(chunk) + c.flush()
        assert len(raw) + 26 <= 65536
        out += (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, len(raw) + 25)
                + raw + struct.pack("<II", zlib.crc32(chunk) & 0xFFFFFFFF, len(chunk)))
    out += bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
    return bytes(out)


def unwrap_fasta(text, device=0):
    """join_fasta(text) computed on the GPU (tsx_hip_unwrap_fasta_host: the whole text as one piece)."""
    b = bytes(text)
    cap = len(b) + 2
    out = ctypes.create_string_buffer(max(cap, 1))
    got = ctypes.c_size_t(0)
    _check(lib().tsx_hip_unwrap_fasta_host(device, b, len(b), out, cap, ctypes.byref(got)))
    return out.raw[:got.value]


def cut_records(text, parts, lines_per_record=4):
    """Where the multi-GPU host cuts a text: parts + 1 offsets, every one a record boundary of the reference's reader."""
    b = bytes(text)
    out = (ctypes.c_size_t * (parts + 1))()
    _check(lib().tsx_hip_cut_records_host(b, len(b), parts, lines_per_record, out))
    return [int(x) for x in out]


def database_info(path_or_fd):
    """The header of a k-mer database file as a dict (tsx_hip_db_read_info; no GPU needed)."""
    info = DbInfo()
    with _fds(path_or_fd, read=True) as (fd,):
        rc = lib().tsx_hip_db_read_info(fd, ctypes.byref(info))
    _check(rc)
    return info.as_dict()


def synth_sizes(seed, first_read, n_reads, k, want_polya=False):
    """Byte and k-mer totals of tsx_hip_synth_fastq_device without generating."""
    nb, nk, npa = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    _check(lib().tsx_hip_synth_fastq_device(seed, first_read, n_reads, k, None, 0, ctypes.byref(nb),
                                            ctypes.byref(nk), ctypes.byref(npa) if want_polya else None, 0, None))
    return int(nb.value), int(nk.value), int(npa.value)


def synth_fastq_device(seed, first_read, n_reads, k, dev_ptr, cap, device=0, stream=None):
    nb, nk = ctypes.c_uint64(0), ctypes.c_uint64(0)
    _check(lib().tsx_hip_synth_fastq_device(seed, first_read, n_reads, k, ctypes.c_void_p(dev_ptr), cap,
                                            ctypes.byref(nb), ctypes.byref(nk), None, device, _stream(stream)))
    return int(nb.value), int(nk.value)


def synth_zipf_device(seed, n_reads, read_len, thr, dev_ptr=None, cap=0, device=0, stream=None):
    """Zipf-skewed reads straight into device memory (tsx_hip_synth_zipf_device; thr from synth.zipf_thresholds).
    Returns the byte count; dev_ptr None = sizing call."""
    thr = np.ascontiguousarray(thr, dtype=np.uint64)
    nb = ctypes.c_uint64(0)
    _check(lib().tsx_hip_synth_zipf_device(seed, n_reads, read_len, len(thr), _p(thr), ctypes.c_void_p(dev_ptr) if dev_ptr else None,
                                           cap, ctypes.byref(nb), device, _stream(stream)))
    return int(nb.value)
