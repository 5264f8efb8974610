// TSXHashMapHIP.h -- host-side C++ mirror of the reference's TSXHashMap surface
// (src/tsxcount/TSXHashMap.h) for --mode=HIP.  Everything below the class is
// the C ABI of libtsxcount_hip.so (include/tsxcount_hip.h); there is no CPU
// counting path in this class.
//
// A reference maintainer would make this `class TSXHashMapHIP : public
// TSXHashMap` and convert UBigInt <-> uint64 limbs at the boundary (see
// INTEGRATION.md); here k-mers are std::vector<uint64_t> limbs in the same
// bit layout UBigInt uses (base i -> bits 2i,2i+1).
#ifndef TSXCOUNT_TSXHASHMAPHIP_H
#define TSXCOUNT_TSXHASHMAPHIP_H

#include <fcntl.h>
#include <unistd.h>

#include <cmath>
#include <cstdint>
#include <exception>
#include <iostream>
#include <string>
#include <utility>
#include <vector>

#include "tsxcount_hip.h"

// TSXException (TSXHashMap.h:28-47)
class TSXException : public std::exception {
public:
    TSXException(std::string sText, int iCode = TSX_HIP_EINVAL) : m_sText(std::move(sText)), m_iCode(iCode) {}
    const char *what() const throw() override { return m_sText.c_str(); }
    int code() const { return m_iCode; }

protected:
    const std::string m_sText;
    const int m_iCode;
};

typedef std::vector<uint64_t> tsx_kmer_t;  // TSX::tsx_kmer_t (TSXTypes.h:23)

// Open (create / truncate) sPath, hand the descriptor to fnWrite (a tsx_hip_*write_counts_host call), close it; fnCheck
// throws on an error code.  Returns the lines written.
template <typename W, typename C>
static uint64_t tsx_write_counts_file(const std::string &sPath, W fnWrite, C fnCheck) {
    const int fd = open(sPath.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (fd < 0) throw TSXException("could not open " + sPath + " for writing", TSX_HIP_EIO);
    uint64_t iLines = 0, iBytes = 0;
    int rc = fnWrite(fd, &iLines, &iBytes);
    if (close(fd) != 0 && rc == TSX_HIP_OK) rc = TSX_HIP_EIO;
    fnCheck(rc);
    return iLines;
}

// Read queries over one table (tsx_hip_query_reads_host / tsx_hip_filter_reads_host); fnCheck throws on an error code.
template <typename C>
static std::vector<tsx_hip_read_stats> tsx_query_reads(tsx_hip_map *pMap, const char *pText, size_t iBytes, uint64_t iLower,
                                                       uint64_t iUpper, size_t iChunkBytes, C fnCheck) {
    // a first guess of 256 bytes per record; a text with shorter records is queried again with the exact count
    std::vector<tsx_hip_read_stats> out(iBytes / 256 + 16);
    size_t n = 0;
    int rc = tsx_hip_query_reads_host(pMap, pText, iBytes, iLower, iUpper, out.data(), out.size(), &n, iChunkBytes);
    if (rc == TSX_HIP_ERANGE) {
        out.resize(n);
        rc = tsx_hip_query_reads_host(pMap, pText, iBytes, iLower, iUpper, out.data(), n, &n, iChunkBytes);
    }
    fnCheck(rc);
    out.resize(n);
    return out;
}
template <typename C>
static std::pair<uint64_t, uint64_t> tsx_filter_reads(tsx_hip_map *pMap, const char *pText, size_t iBytes,
                                                      const tsx_hip_filter_rule &oRule, const std::string &sPath,
                                                      size_t iChunkBytes, C fnCheck) {
    const int fd = open(sPath.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (fd < 0) throw TSXException("could not open " + sPath + " for writing", TSX_HIP_EIO);
    uint64_t iKept = 0, iWritten = 0;
    int rc = tsx_hip_filter_reads_host(pMap, pText, iBytes, &oRule, fd, iChunkBytes, &iKept, &iWritten);
    if (close(fd) != 0 && rc == TSX_HIP_OK) rc = TSX_HIP_EIO;
    fnCheck(rc);
    return std::make_pair(iKept, iWritten);
}
// Sequence queries over one table (tsx_hip_seq_*): the result of one call, freed with the object.
struct TSXSequenceResult {
    tsx_hip_seq_result *p = nullptr;
    TSXSequenceResult() = default;
    TSXSequenceResult(const TSXSequenceResult &) = delete;
    TSXSequenceResult &operator=(const TSXSequenceResult &) = delete;
    TSXSequenceResult(TSXSequenceResult &&o) : p(o.p) { o.p = nullptr; }
    TSXSequenceResult &operator=(TSXSequenceResult &&o) {
        if (this != &o) { tsx_hip_seq_result_free(p); p = o.p; o.p = nullptr; }
        return *this;
    }
    ~TSXSequenceResult() { tsx_hip_seq_result_free(p); }
    size_t size() const { return tsx_hip_seq_result_count(p); }
    const tsx_hip_seq_stats *stats() const { return tsx_hip_seq_result_stats(p); }
    std::string name(size_t i) const {
        const uint64_t *off = nullptr;
        const char *blob = tsx_hip_seq_result_names(p, &off);
        if (!blob || !off || i >= size()) return std::string();
        return std::string(blob + off[i], (size_t)(off[i + 1] - off[i]));
    }
    std::vector<tsx_hip_seq_interval> intervals() const {
        const tsx_hip_seq_interval *iv = nullptr;
        const size_t n = tsx_hip_seq_result_intervals(p, &iv);
        return std::vector<tsx_hip_seq_interval>(iv, iv + n);
    }
    // a track (sequenceTrack): its window, 0 without one; the bins of sequence i
    uint64_t window() const { return tsx_hip_seq_result_window(p); }
    std::vector<tsx_hip_seq_bin> bins(size_t i) const {
        const tsx_hip_seq_bin *b = nullptr;
        const uint64_t *first = nullptr;
        tsx_hip_seq_result_bins(p, &b, &first);
        if (!b || !first || i >= size()) return std::vector<tsx_hip_seq_bin>();
        return std::vector<tsx_hip_seq_bin>(b + first[i], b + first[i + 1]);
    }
};
// bBgzf: pText is the image of a BGZF file; bMissing: the intervals too
template <typename C>
static TSXSequenceResult tsx_query_sequences(tsx_hip_map *pMap, const char *pText, size_t iBytes, bool bBgzf, bool bMissing,
                                             uint64_t iLower, uint64_t iUpper, size_t iChunkBytes, C fnCheck) {
    TSXSequenceResult r;
    int rc;
    if (bBgzf) rc = bMissing ? tsx_hip_seq_missing_bgzf_host(pMap, pText, iBytes, iLower, iUpper, &r.p)
                             : tsx_hip_seq_stats_bgzf_host(pMap, pText, iBytes, iLower, iUpper, &r.p);
    else rc = bMissing ? tsx_hip_seq_missing_host(pMap, pText, iBytes, iLower, iUpper, iChunkBytes, &r.p)
                       : tsx_hip_seq_stats_host(pMap, pText, iBytes, iLower, iUpper, iChunkBytes, &r.p);
    fnCheck(rc);
    return r;
}
// a result into sPath (created / truncated) through fnWrite(fd)
template <typename W, typename C>
static void tsx_write_sequence_file(const std::string &sPath, W fnWrite, C fnCheck) {
    const int fd = open(sPath.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (fd < 0) throw TSXException("could not open " + sPath + " for writing", TSX_HIP_EIO);
    int rc = fnWrite(fd);
    if (close(fd) != 0 && rc == TSX_HIP_OK) rc = TSX_HIP_EIO;
    fnCheck(rc);
}
// name, length, kmers, present, missing, min, sum, qv per sequence
template <typename C>
static void tsx_write_sequence_stats(const TSXSequenceResult &r, int iK, const std::string &sPath, C fnCheck) {
    tsx_write_sequence_file(sPath, [&](int fd) { return tsx_hip_seq_write_stats(r.p, iK, fd); }, fnCheck);
}
// the missing intervals as BED
template <typename C>
static void tsx_write_sequence_missing(const TSXSequenceResult &r, const std::string &sPath, C fnCheck) {
    tsx_write_sequence_file(sPath, [&](int fd) { return tsx_hip_seq_write_missing(r.p, fd); }, fnCheck);
}
// the coverage track of a wrapped FASTA text (tsx_hip_seq_track_host) and its file: one line per bin
template <typename C>
static TSXSequenceResult tsx_sequence_track(tsx_hip_map *pMap, const char *pText, size_t iBytes, uint64_t iWindow, uint64_t iLower,
                                            uint64_t iUpper, size_t iChunkBytes, C fnCheck) {
    TSXSequenceResult r;
    fnCheck(tsx_hip_seq_track_host(pMap, pText, iBytes, iLower, iUpper, iWindow, iChunkBytes, &r.p));
    return r;
}
template <typename C>
static void tsx_write_sequence_track(const TSXSequenceResult &r, const std::string &sPath, C fnCheck) {
    tsx_write_sequence_file(sPath, [&](int fd) { return tsx_hip_seq_write_track(r.p, fd); }, fnCheck);
}
// Read trimming over one table (tsx_hip_trim_spans_host / tsx_hip_trim_reads_host).
template <typename C>
static std::vector<tsx_hip_trim_span> tsx_trim_spans(tsx_hip_map *pMap, const char *pText, size_t iBytes,
                                                     const tsx_hip_trim_rule &oRule, size_t iChunkBytes, C fnCheck) {
    std::vector<tsx_hip_trim_span> out(iBytes / 256 + 16);
    size_t n = 0;
    int rc = tsx_hip_trim_spans_host(pMap, pText, iBytes, &oRule, out.data(), out.size(), &n, iChunkBytes);
    if (rc == TSX_HIP_ERANGE) {
        out.resize(n);
        rc = tsx_hip_trim_spans_host(pMap, pText, iBytes, &oRule, out.data(), n, &n, iChunkBytes);
    }
    fnCheck(rc);
    out.resize(n);
    return out;
}
template <typename C>
static tsx_hip_trim_totals tsx_trim_reads(tsx_hip_map *pMap, const char *pText, size_t iBytes, const tsx_hip_trim_rule &oRule,
                                          const std::string &sPath, size_t iChunkBytes, C fnCheck) {
    const int fd = open(sPath.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (fd < 0) throw TSXException("could not open " + sPath + " for writing", TSX_HIP_EIO);
    tsx_hip_trim_totals oTotals = {0, 0, 0, 0, 0};
    int rc = tsx_hip_trim_reads_host(pMap, pText, iBytes, &oRule, fd, iChunkBytes, &oTotals);
    if (close(fd) != 0 && rc == TSX_HIP_OK) rc = TSX_HIP_EIO;
    fnCheck(rc);
    return oTotals;
}
// Read medians over one table (tsx_hip_count_profile_host / tsx_hip_median_reads_host / tsx_hip_filter_median_host).
template <typename C>
static std::vector<uint32_t> tsx_count_profile(tsx_hip_map *pMap, const char *pText, size_t iBytes, size_t iChunkBytes, C fnCheck) {
    std::vector<uint32_t> out(iBytes);
    fnCheck(tsx_hip_count_profile_host(pMap, pText, iBytes, out.data(), iChunkBytes));
    return out;
}
template <typename C>
static std::vector<tsx_hip_read_median> tsx_median_reads(tsx_hip_map *pMap, const char *pText, size_t iBytes, size_t iChunkBytes,
                                                         C fnCheck) {
    std::vector<tsx_hip_read_median> out(iBytes / 256 + 16);
    size_t n = 0;
    int rc = tsx_hip_median_reads_host(pMap, pText, iBytes, out.data(), out.size(), &n, iChunkBytes);
    if (rc == TSX_HIP_ERANGE) {
        out.resize(n);
        rc = tsx_hip_median_reads_host(pMap, pText, iBytes, out.data(), n, &n, iChunkBytes);
    }
    fnCheck(rc);
    out.resize(n);
    return out;
}
template <typename C>
static std::pair<uint64_t, uint64_t> tsx_filter_median(tsx_hip_map *pMap, const char *pText, size_t iBytes,
                                                       const tsx_hip_median_rule &oRule, const std::string &sPath,
                                                       size_t iChunkBytes, C fnCheck) {
    const int fd = open(sPath.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (fd < 0) throw TSXException("could not open " + sPath + " for writing", TSX_HIP_EIO);
    uint64_t iKept = 0, iWritten = 0;
    int rc = tsx_hip_filter_median_host(pMap, pText, iBytes, &oRule, fd, iChunkBytes, &iKept, &iWritten);
    if (close(fd) != 0 && rc == TSX_HIP_OK) rc = TSX_HIP_EIO;
    fnCheck(rc);
    return std::make_pair(iKept, iWritten);
}
// Digital normalization (tsx_hip_normalize_host): the kept records into sPath (created / truncated; empty: no output).
template <typename C>
static tsx_hip_normalize_totals tsx_normalize_reads(tsx_hip_map *pMap, const char *pText, size_t iBytes,
                                                    const tsx_hip_normalize_rule &oRule, const std::string &sPath,
                                                    size_t iChunkBytes, C fnCheck) {
    int fd = -1;
    if (!sPath.empty()) {
        fd = open(sPath.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
        if (fd < 0) throw TSXException("could not open " + sPath + " for writing", TSX_HIP_EIO);
    }
    tsx_hip_normalize_totals oTotals;
    int rc = tsx_hip_normalize_host(pMap, pText, iBytes, &oRule, fd, nullptr, 0, iChunkBytes, &oTotals);
    if (fd >= 0 && close(fd) != 0 && rc == TSX_HIP_OK) rc = TSX_HIP_EIO;
    if (rc == TSX_HIP_EINVAL) throw TSXException(std::string("normalize: ") + tsx_hip_last_error(), rc);
    fnCheck(rc);
    return oTotals;
}
// The filter and the trim over mate pairs (tsx_hip_filter_pairs_host / tsx_hip_trim_pairs_host).  pText2 == nullptr: one
// interleaved text.  Paths: kept mates 1, kept mates 2, orphans of text 1, orphans of text 2 -- created / truncated; an
// empty path is no output (-1: allowed for the orphans, and for everything of text 2 with an interleaved text).
// fnCall(io, totals) makes the call.
template <typename F, typename C>
static tsx_hip_pair_totals tsx_pairs_files(const std::string (&sPaths)[4], F fnCall, C fnCheck) {
    int fds[4] = {-1, -1, -1, -1};
    for (int i = 0; i < 4; ++i) {
        if (sPaths[i].empty()) continue;
        fds[i] = open(sPaths[i].c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
        if (fds[i] < 0) {
            for (int j = 0; j < i; ++j) if (fds[j] >= 0) close(fds[j]);
            throw TSXException("could not open " + sPaths[i] + " for writing", TSX_HIP_EIO);
        }
    }
    const tsx_hip_pair_io io = {fds[0], fds[1], fds[2], fds[3]};
    tsx_hip_pair_totals oTotals = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    int rc = fnCall(&io, &oTotals);
    for (int i = 0; i < 4; ++i)
        if (fds[i] >= 0 && close(fds[i]) != 0 && rc == TSX_HIP_OK) rc = TSX_HIP_EIO;
    fnCheck(rc);
    return oTotals;
}
template <typename C>
static tsx_hip_pair_totals tsx_filter_pairs(tsx_hip_map *pMap, const char *pText1, size_t iBytes1, const char *pText2, size_t iBytes2,
                                            const tsx_hip_filter_rule &oRule, int iPairMode, bool bCheckNames,
                                            const std::string (&sPaths)[4], size_t iChunkBytes, C fnCheck) {
    return tsx_pairs_files(sPaths, [&](const tsx_hip_pair_io *io, tsx_hip_pair_totals *t) {
        return tsx_hip_filter_pairs_host(pMap, pText1, iBytes1, pText2, iBytes2, &oRule, iPairMode, bCheckNames ? 1 : 0, io, iChunkBytes, t);
    }, fnCheck);
}
template <typename C>
static tsx_hip_pair_totals tsx_trim_pairs(tsx_hip_map *pMap, const char *pText1, size_t iBytes1, const char *pText2, size_t iBytes2,
                                          const tsx_hip_trim_rule &oRule, bool bCheckNames, const std::string (&sPaths)[4],
                                          size_t iChunkBytes, C fnCheck) {
    return tsx_pairs_files(sPaths, [&](const tsx_hip_pair_io *io, tsx_hip_pair_totals *t) {
        return tsx_hip_trim_pairs_host(pMap, pText1, iBytes1, pText2, iBytes2, &oRule, bCheckNames ? 1 : 0, io, iChunkBytes, t);
    }, fnCheck);
}

class TSXHashMapHIP {
public:
    // TSXHashMapCAS(iL, iStorageBits, iK, iThreads) (TSXHashMapCAS.h:239-245);
    // iThreads is accepted for CLI compatibility, the GPU picks its own launch width.
    TSXHashMapHIP(uint8_t iL, uint32_t iStorageBits, uint16_t iK, uint8_t iThreads = 0, uint64_t iHashSeed = 1,
                  int iDevice = 0, int iOverflowL = 0)
        : m_iL(iL), m_iK(iK), m_iThreads(iThreads) {
        int rc = tsx_hip_create(&m_pMap, iK, iL, (int)iStorageBits, iOverflowL, iHashSeed, iDevice);
        check(rc);
        check(tsx_hip_get_layout(m_pMap, &m_oLayout));
        std::cerr << "Creating array with " << m_oLayout.table_bytes << " bytes for " << m_oLayout.slots
                  << " places." << std::endl;
        std::cerr << "Maximum number of allowed reprobes per element: " << m_oLayout.max_reprobes << std::endl;
    }
    ~TSXHashMapHIP() { tsx_hip_destroy(m_pMap); }
    TSXHashMapHIP(const TSXHashMapHIP &) = delete;
    TSXHashMapHIP &operator=(const TSXHashMapHIP &) = delete;

    uint64_t getMaxElements() const { return m_oLayout.slots; }  // TSXHashMap.h:162
    uint32_t getK() const { return m_iK; }                       // TSXHashMap.h:172
    int getThreads() const { return m_iThreads; }                // TSXHashMap.h:737
    const tsx_hip_layout &getLayout() const { return m_oLayout; }

    // TSXSeqUtils::fromSequence (SequenceUtils.h:86-160)
    tsx_kmer_t fromSequence(const std::string &seq) const {
        tsx_kmer_t out(m_oLayout.key_limbs);
        check(tsx_hip_encode(seq.c_str(), m_iK, out.data()));
        return out;
    }
    // TSXSeqUtils::toSequence (SequenceUtils.h:47-84)
    std::string toSequence(const tsx_kmer_t &kmer) const {
        std::string s(m_iK + 1, '\0');
        check(tsx_hip_decode(kmer.data(), m_iK, &s[0]));
        s.resize(m_iK);
        return s;
    }

    // addKmer (TSXHashMap.h:182); batches go through addKmers.
    bool addKmer(const tsx_kmer_t &kmer) {
        check(tsx_hip_add_kmers_host(m_pMap, kmer.data(), nullptr, 1));
        return true;
    }
    void addKmers(const std::vector<uint64_t> &limbs, size_t n, const uint64_t *counts = nullptr) {
        check(tsx_hip_add_kmers_host(m_pMap, limbs.data(), counts, n));
    }

    // getKmerCount(kmer) (TSXHashMap.h:548)
    uint64_t getKmerCount(const tsx_kmer_t &kmer) {
        uint64_t c = 0;
        check(tsx_hip_get_counts_host(m_pMap, kmer.data(), 1, &c));
        return c;
    }
    void getKmerCounts(const std::vector<uint64_t> &limbs, size_t n, std::vector<uint64_t> &out) {
        out.resize(n);
        check(tsx_hip_get_counts_host(m_pMap, limbs.data(), n, out.data()));
    }
    // getKmerCount() (TSXHashMap.h:645)
    uint64_t getKmerCount() { return stats().distinct; }

    // getAllKmers (TSXHashMap.h:660), with counts
    std::vector<tsx_kmer_t> getAllKmers(std::vector<uint64_t> *pCounts = nullptr) {
        size_t n = (size_t)stats().distinct, got = 0;
        std::vector<uint64_t> limbs((n ? n : 1) * m_oLayout.key_limbs), counts(n ? n : 1);
        check(tsx_hip_dump_host(m_pMap, limbs.data(), counts.data(), n ? n : 1, &got));
        std::vector<tsx_kmer_t> out(got);
        for (size_t i = 0; i < got; ++i)
            out[i].assign(limbs.begin() + i * m_oLayout.key_limbs, limbs.begin() + (i + 1) * m_oLayout.key_limbs);
        if (pCounts) { counts.resize(got); *pCounts = counts; }
        return out;
    }

    // abundance histogram: [c] = k-mers counted c times, [iBins - 1] = counted iBins - 1 times or more
    std::vector<uint64_t> histogram(size_t iBins) {
        std::vector<uint64_t> h(iBins);
        check(tsx_hip_histogram_host(m_pMap, h.data(), iBins));
        return h;
    }
    // the FASTQ.<k>.count file main.cpp:224-396 reads: "kmer<TAB>count" for every count in [iLower, iUpper]; returns lines
    uint64_t write_counts(const std::string &sPath, uint64_t iLower = 1, uint64_t iUpper = UINT64_MAX) {
        return tsx_write_counts_file(sPath, [&](int fd, uint64_t *l, uint64_t *b) {
            return tsx_hip_write_counts_host(m_pMap, fd, iLower, iUpper, 0, l, b);
        }, check);
    }

    // the table as a k-mer database file (tsx_hip_save_host), created / truncated; returns the entries written
    uint64_t saveDatabase(const std::string &sPath, size_t iChunkBytes = 0) {
        return tsx_write_counts_file(sPath, [&](int fd, uint64_t *e, uint64_t *b) {
            return tsx_hip_save_host(m_pMap, fd, iChunkBytes, e, b);
        }, check);
    }
    // a k-mer database into this table (tsx_hip_load_host): placed as it is, or added to what the table holds; returns the
    // entries read
    uint64_t loadDatabase(const std::string &sPath, size_t iChunkBytes = 0) {
        const int fd = open(sPath.c_str(), O_RDONLY);
        if (fd < 0) throw TSXException("could not open " + sPath, TSX_HIP_EIO);
        uint64_t iEntries = 0;
        const int rc = tsx_hip_load_host(m_pMap, fd, iChunkBytes, &iEntries);
        close(fd);
        check(rc);
        return iEntries;
    }
    // the header of a k-mer database file (tsx_hip_db_read_info; no GPU)
    static tsx_hip_db_info databaseInfo(const std::string &sPath) {
        const int fd = open(sPath.c_str(), O_RDONLY);
        if (fd < 0) throw TSXException("could not open " + sPath, TSX_HIP_EIO);
        tsx_hip_db_info oInfo;
        const int rc = tsx_hip_db_read_info(fd, &oInfo);
        close(fd);
        check(rc);
        return oInfo;
    }

    // per-record k-mer stats of a text against the table, records in text order (tsx_hip_query_reads_host)
    std::vector<tsx_hip_read_stats> queryReads(const char *pText, size_t iBytes, uint64_t iLower = 1,
                                               uint64_t iUpper = UINT64_MAX, size_t iChunkBytes = 0) {
        return tsx_query_reads(m_pMap, pText, iBytes, iLower, iUpper, iChunkBytes, check);
    }
    // the records of a text that pass oRule into sPath (created / truncated); returns {records kept, bytes written}
    std::pair<uint64_t, uint64_t> filterReads(const char *pText, size_t iBytes, const tsx_hip_filter_rule &oRule,
                                              const std::string &sPath, size_t iChunkBytes = 0) {
        return tsx_filter_reads(m_pMap, pText, iBytes, oRule, sPath, iChunkBytes, check);
    }
    // per-sequence stats and names of a wrapped FASTA text against the table (tsx_hip_seq_stats_host)
    TSXSequenceResult querySequences(const char *pText, size_t iBytes, uint64_t iLower = 1, uint64_t iUpper = UINT64_MAX,
                                     size_t iChunkBytes = 0) {
        return tsx_query_sequences(m_pMap, pText, iBytes, false, false, iLower, iUpper, iChunkBytes, check);
    }
    // the same with the maximal runs of missing k-mers (tsx_hip_seq_missing_host)
    TSXSequenceResult missingIntervals(const char *pText, size_t iBytes, uint64_t iLower = 1, uint64_t iUpper = UINT64_MAX,
                                       size_t iChunkBytes = 0) {
        return tsx_query_sequences(m_pMap, pText, iBytes, false, true, iLower, iUpper, iChunkBytes, check);
    }
    // name, length, kmers, present, missing, min, sum, qv per sequence into sPath; returns the sequences
    size_t writeSequenceStats(const char *pText, size_t iBytes, const std::string &sPath, uint64_t iLower = 1,
                              uint64_t iUpper = UINT64_MAX, size_t iChunkBytes = 0) {
        const TSXSequenceResult r = querySequences(pText, iBytes, iLower, iUpper, iChunkBytes);
        tsx_write_sequence_stats(r, (int)getK(), sPath, check);
        return r.size();
    }
    // the missing intervals as BED (name, start, end) into sPath; returns the intervals
    size_t writeMissing(const char *pText, size_t iBytes, const std::string &sPath, uint64_t iLower = 1,
                        uint64_t iUpper = UINT64_MAX, size_t iChunkBytes = 0) {
        const TSXSequenceResult r = missingIntervals(pText, iBytes, iLower, iUpper, iChunkBytes);
        tsx_write_sequence_missing(r, sPath, check);
        return r.intervals().size();
    }
    // the coverage track: stats and names as querySequences, and per sequence its bins of iWindow start positions
    TSXSequenceResult sequenceTrack(const char *pText, size_t iBytes, uint64_t iWindow, uint64_t iLower = 1,
                                    uint64_t iUpper = UINT64_MAX, size_t iChunkBytes = 0) {
        return tsx_sequence_track(m_pMap, pText, iBytes, iWindow, iLower, iUpper, iChunkBytes, check);
    }
    // name, start, end, kmers, present, min, max, mean per bin into sPath; returns the sequences
    size_t writeSequenceTrack(const char *pText, size_t iBytes, const std::string &sPath, uint64_t iWindow, uint64_t iLower = 1,
                              uint64_t iUpper = UINT64_MAX, size_t iChunkBytes = 0) {
        const TSXSequenceResult r = sequenceTrack(pText, iBytes, iWindow, iLower, iUpper, iChunkBytes);
        tsx_write_sequence_track(r, sPath, check);
        return r.size();
    }
    // the count of every window of a text, one entry per byte (TSX_HIP_NO_KMER where no k-mer starts)
    std::vector<uint32_t> countProfile(const char *pText, size_t iBytes, size_t iChunkBytes = 0) {
        return tsx_count_profile(m_pMap, pText, iBytes, iChunkBytes, check);
    }
    // {kmers, median} of every record of a text (tsx_hip_median_reads_host)
    std::vector<tsx_hip_read_median> medianReads(const char *pText, size_t iBytes, size_t iChunkBytes = 0) {
        return tsx_median_reads(m_pMap, pText, iBytes, iChunkBytes, check);
    }
    // the records of a text whose median passes oRule into sPath (created / truncated); returns {records kept, bytes written}
    std::pair<uint64_t, uint64_t> filterByMedian(const char *pText, size_t iBytes, const tsx_hip_median_rule &oRule,
                                                 const std::string &sPath, size_t iChunkBytes = 0) {
        return tsx_filter_median(m_pMap, pText, iBytes, oRule, sPath, iChunkBytes, check);
    }
    // digital normalization: records kept while their median is below iCutoff, in rounds of iRoundRecords; the kept
    // records into sPath (empty: no output), their k-mers into the table; returns the totals
    tsx_hip_normalize_totals normalizeReads(const char *pText, size_t iBytes, uint64_t iCutoff = 20,
                                            uint64_t iRoundRecords = TSX_HIP_NORMALIZE_ROUND, const std::string &sPath = std::string(),
                                            size_t iChunkBytes = 0) {
        const tsx_hip_normalize_rule oRule = {iCutoff, iRoundRecords, {0, 0}};
        return tsx_normalize_reads(m_pMap, pText, iBytes, oRule, sPath, iChunkBytes, check);
    }
    // the kept span (start, length) of every record of a text under oRule (tsx_hip_trim_spans_host)
    std::vector<tsx_hip_trim_span> trimSpans(const char *pText, size_t iBytes, const tsx_hip_trim_rule &oRule,
                                             size_t iChunkBytes = 0) {
        return tsx_trim_spans(m_pMap, pText, iBytes, oRule, iChunkBytes, check);
    }
    // the records of a text cut to their kept spans into sPath (created / truncated); returns the totals
    tsx_hip_trim_totals trimReads(const char *pText, size_t iBytes, const tsx_hip_trim_rule &oRule, const std::string &sPath,
                                  size_t iChunkBytes = 0) {
        return tsx_trim_reads(m_pMap, pText, iBytes, oRule, sPath, iChunkBytes, check);
    }
    // the single substitutions the spectrum undoes in a text (tsx_hip_correct_sites_host), sorted by (record, pos)
    std::vector<tsx_hip_correction> correctionSites(const char *pText, size_t iBytes, const tsx_hip_correct_rule &oRule,
                                                    tsx_hip_correct_totals *pTotals = nullptr, size_t iChunkBytes = 0) {
        std::vector<tsx_hip_correction> out(iBytes / 256 + 16);
        size_t n = 0;
        int rc = tsx_hip_correct_sites_host(m_pMap, pText, iBytes, &oRule, out.data(), out.size(), &n, pTotals, iChunkBytes);
        if (rc == TSX_HIP_ERANGE) {
            out.resize(n);
            rc = tsx_hip_correct_sites_host(m_pMap, pText, iBytes, &oRule, out.data(), n, &n, pTotals, iChunkBytes);
        }
        check(rc);
        out.resize(n);
        return out;
    }
    // the text with them applied, byte for byte as long, to an open descriptor (tsx_hip_correct_reads_host)
    tsx_hip_correct_totals correctReads(const char *pText, size_t iBytes, int iFd, const tsx_hip_correct_rule &oRule,
                                        size_t iChunkBytes = 0) {
        tsx_hip_correct_totals t = {0, 0, 0, 0, 0, 0};
        check(tsx_hip_correct_reads_host(m_pMap, pText, iBytes, &oRule, iFd, iChunkBytes, &t));
        return t;
    }
    // the filter / the trim over mate pairs (pText2 == nullptr: interleaved); sPaths as tsx_pairs_files takes them
    tsx_hip_pair_totals filterPairs(const char *pText1, size_t iBytes1, const char *pText2, size_t iBytes2,
                                    const tsx_hip_filter_rule &oRule, const std::string (&sPaths)[4],
                                    int iPairMode = TSX_HIP_PAIR_BOTH, bool bCheckNames = false, size_t iChunkBytes = 0) {
        return tsx_filter_pairs(m_pMap, pText1, iBytes1, pText2, iBytes2, oRule, iPairMode, bCheckNames, sPaths, iChunkBytes, check);
    }
    tsx_hip_pair_totals trimPairs(const char *pText1, size_t iBytes1, const char *pText2, size_t iBytes2,
                                  const tsx_hip_trim_rule &oRule, const std::string (&sPaths)[4], bool bCheckNames = false,
                                  size_t iChunkBytes = 0) {
        return tsx_trim_pairs(m_pMap, pText1, iBytes1, pText2, iBytes2, oRule, bCheckNames, sPaths, iChunkBytes, check);
    }

    // table sizing (tsx_hip_sketch_*): the HyperLogLog registers of the k-mers a text would put into a table, max-combined
    // into oRegs (2^iPrecision entries; an empty vector is sized and zeroed); returns the totals, added to *pTotals too.
    // This map supplies k, the record lines, canonical and the base rule; its table is neither read nor written.
    tsx_hip_sketch_totals sketchKmers(const char *pText, size_t iBytes, std::vector<uint8_t> &oRegs, int iPrecision = 14,
                                      size_t iChunkBytes = 0) {
        tsx_hip_sketch_totals t = {0, 0};
        if (oRegs.empty() && iPrecision >= 0 && iPrecision < 31) oRegs.assign((size_t)1 << iPrecision, 0);
        if (oRegs.size() != ((size_t)1 << (iPrecision & 31))) check(TSX_HIP_EINVAL);
        check(tsx_hip_sketch_host(m_pMap, pText, iBytes, iPrecision, oRegs.data(), &t, iChunkBytes));
        return t;
    }
    tsx_hip_sketch_totals sketchKmersBgzf(const void *pGz, size_t iBytes, std::vector<uint8_t> &oRegs, int iPrecision = 14) {
        tsx_hip_sketch_totals t = {0, 0};
        if (oRegs.empty() && iPrecision >= 0 && iPrecision < 31) oRegs.assign((size_t)1 << iPrecision, 0);
        if (oRegs.size() != ((size_t)1 << (iPrecision & 31))) check(TSX_HIP_EINVAL);
        const int rc = tsx_hip_sketch_bgzf_host(m_pMap, pGz, iBytes, iPrecision, oRegs.data(), &t);
        if (rc == TSX_HIP_EINVAL && *tsx_hip_last_error()) throw TSXException(std::string("BGZF input: ") + tsx_hip_last_error(), rc);
        check(rc);
        return t;
    }
    // counting only the k-mers seen twice (tsx_hip_prefilter_*): pass 1 puts the k-mers of a text into the map's prefilter
    // (iBits != 0: a new filter of 2^iBits bits first; 0: the one the map has -- several texts accumulate); while armed,
    // the FASTQ counting calls insert only what the filter has seen twice.  After both passes over the same input every
    // k-mer that occurs twice has its exact count; one that occurs once is absent or, seldom, there with count 1.
    void prefilter(const char *pText, size_t iBytes, int iBits = 0, size_t iChunkBytes = 0) {
        if (iBits) check(tsx_hip_prefilter_create(m_pMap, iBits));
        check(tsx_hip_prefilter_add_host(m_pMap, pText, iBytes, iChunkBytes));
    }
    void prefilterBgzf(const void *pGz, size_t iBytes, int iBits = 0) {
        if (iBits) check(tsx_hip_prefilter_create(m_pMap, iBits));
        const int rc = tsx_hip_prefilter_add_bgzf_host(m_pMap, pGz, iBytes);
        if (rc == TSX_HIP_EINVAL && *tsx_hip_last_error()) throw TSXException(std::string("BGZF input: ") + tsx_hip_last_error(), rc);
        check(rc);
    }
    void armPrefilter(bool bOn = true) { check(tsx_hip_prefilter_arm(m_pMap, bOn ? 1 : 0)); }
    tsx_hip_prefilter_totals prefilterStats() {
        tsx_hip_prefilter_totals t;
        check(tsx_hip_prefilter_stats(m_pMap, &t));
        return t;
    }
    // the distinct k-mers a sketch stands for (tsx_hip_sketch_estimate_host)
    static double estimate(const std::vector<uint8_t> &oRegs) {
        int p = 0;
        while (p < 31 && ((size_t)1 << p) < oRegs.size()) ++p;
        const double e = (((size_t)1 << p) == oRegs.size()) ? tsx_hip_sketch_estimate_host(oRegs.data(), p) : -1.0;
        if (e < 0) check(TSX_HIP_EINVAL);
        return e;
    }
    // the l that holds dDistinct k-mers at load dLoad with five standard errors of margin (tsx_hip_suggest_l); *pClamped:
    // the bounds on l left the load above 0.9 (TSX_HIP_ERANGE), which throws when pClamped is null
    static int suggestL(int iK, double dDistinct, double dLoad = 0.75, int iPrecision = 14, bool *pClamped = nullptr) {
        int l = 0;
        const int rc = tsx_hip_suggest_l(iK, dDistinct, iPrecision, (uint32_t)std::llround(dLoad * 1e6), &l);
        if (pClamped) *pClamped = rc == TSX_HIP_ERANGE;
        if (rc != TSX_HIP_ERANGE || !pClamped) check(rc);
        return l;
    }

    // set operation on two tables (tsx_hip_combine): this is A, oOther is B, the result goes into the empty table oOut
    tsx_hip_combine_stats combine(TSXHashMapHIP &oOther, TSXHashMapHIP &oOut, const tsx_hip_combine_rule &oRule) {
        return combineInto(oOut.m_pMap, oOther, oRule);
    }
    // how two tables overlap: the stats of an intersection, nothing is written (jaccard() turns them into the index)
    tsx_hip_combine_stats compare(TSXHashMapHIP &oOther, uint64_t iALower = 1, uint64_t iAUpper = UINT64_MAX,
                                  uint64_t iBLower = 1, uint64_t iBUpper = UINT64_MAX) {
        const tsx_hip_combine_rule oRule = {TSX_HIP_OP_INTERSECT, TSX_HIP_CNT_MIN, iALower, iAUpper, iBLower, iBUpper};
        return combineInto(nullptr, oOther, oRule);
    }
    static double jaccard(const tsx_hip_combine_stats &s) {
        const uint64_t iUnion = s.a_in_range + s.b_in_range - s.both;
        return iUnion ? (double)s.both / (double)iUnion : 0.0;
    }
    // joint spectrum of two tables (tsx_hip_joint_histogram_host): this is A, oOther is B; oMatrix[i * iNb + j] = distinct
    // k-mers counted i times here and j times there, the last bin of each side pooling every larger count
    void jointHistogram(TSXHashMapHIP &oOther, size_t iNa, size_t iNb, std::vector<uint64_t> &oMatrix) {
        oMatrix.assign(iNa && iNb <= ((size_t)1 << 24) / iNa ? iNa * iNb : 0, 0);   // (a refused size allocates nothing)
        const int rc = tsx_hip_joint_histogram_host(m_pMap, oOther.m_pMap, oMatrix.data(), iNa, iNb);
        if (rc == TSX_HIP_EINVAL) throw TSXException(tsx_hip_last_error(), rc);   // (the refusal says which argument)
        check(rc);
    }

    // heterozygous k-mer pairs of this table (tsx_hip_het_histogram_host): oMatrix[i * iNmajor + j] = pairs of k-mers that
    // differ only in their middle base, counted i (the lower count) and j times, the last bin of each side pooling every
    // larger count; k must be odd
    tsx_hip_het_stats hetHistogram(const tsx_hip_het_rule &oRule, size_t iNminor, size_t iNmajor, std::vector<uint64_t> &oMatrix) {
        oMatrix.assign(iNminor && iNmajor <= ((size_t)1 << 24) / iNminor ? iNminor * iNmajor : 0, 0);   // (a refused size allocates nothing)
        tsx_hip_het_stats s = {0, 0, 0, 0, 0};
        const int rc = tsx_hip_het_histogram_host(m_pMap, &oRule, oMatrix.data(), iNminor, iNmajor, &s);
        if (rc == TSX_HIP_EINVAL) throw TSXException(tsx_hip_last_error(), rc);   // (the refusal says which argument)
        check(rc);
        return s;
    }
    // the pairs as minor_kmer<TAB>minor_count<TAB>major_kmer<TAB>major_count lines, the file created / truncated; returns the pairs
    uint64_t writeHetPairs(const std::string &sPath, const tsx_hip_het_rule &oRule) {
        return tsx_write_counts_file(sPath, [&](int fd, uint64_t *l, uint64_t *b) {
            return tsx_hip_write_het_pairs_host(m_pMap, &oRule, fd, 0, l, b);
        }, [&](int rc) {
            if (rc == TSX_HIP_EINVAL) throw TSXException(tsx_hip_last_error(), rc);
            check(rc);
        });
    }

    // unitigs of this table, the compacted de Bruijn graph (tsx_hip_unitig_stats): the totals alone, nothing spelled
    tsx_hip_unitig_totals unitigStats(const tsx_hip_unitig_rule &oRule) {
        tsx_hip_unitig_totals t = tsx_hip_unitig_totals();
        const int rc = tsx_hip_unitig_stats(m_pMap, &oRule, &t);
        if (rc == TSX_HIP_EINVAL) throw TSXException(tsx_hip_last_error(), rc);   // (the refusal says which argument)
        check(rc);
        return t;
    }
    // the unitigs themselves (tsx_hip_unitigs_host): the sequence of record r is sSeq.substr(r.offset, r.length); a first
    // guess of the room, then once more with the sizes the library reports
    tsx_hip_unitig_totals unitigs(const tsx_hip_unitig_rule &oRule, std::string &sSeq, std::vector<tsx_hip_unitig> &oRecords) {
        tsx_hip_unitig_totals t = tsx_hip_unitig_totals();
        size_t n = 0, iBytes = 0;
        sSeq.assign((size_t)1 << 18, '\0');
        oRecords.assign((size_t)1 << 12, tsx_hip_unitig());
        int rc = tsx_hip_unitigs_host(m_pMap, &oRule, &sSeq[0], sSeq.size(), oRecords.data(), oRecords.size(), &n, &iBytes, &t);
        if (rc == TSX_HIP_ERANGE) {
            sSeq.assign(iBytes + 1, '\0');
            oRecords.assign(n + 1, tsx_hip_unitig());
            rc = tsx_hip_unitigs_host(m_pMap, &oRule, &sSeq[0], sSeq.size(), oRecords.data(), oRecords.size(), &n, &iBytes, &t);
        }
        if (rc == TSX_HIP_EINVAL) throw TSXException(tsx_hip_last_error(), rc);
        check(rc);
        sSeq.resize(iBytes);
        oRecords.resize(n);
        return t;
    }
    // the unitigs as FASTA with BCALM's header (tsx_hip_write_unitigs_host), the file created / truncated
    tsx_hip_unitig_totals writeUnitigs(const std::string &sPath, const tsx_hip_unitig_rule &oRule) {
        tsx_hip_unitig_totals t = tsx_hip_unitig_totals();
        tsx_write_counts_file(sPath, [&](int fd, uint64_t *, uint64_t *) {
            return tsx_hip_write_unitigs_host(m_pMap, &oRule, fd, &t);
        }, [&](int rc) {
            if (rc == TSX_HIP_EINVAL) throw TSXException(tsx_hip_last_error(), rc);
            check(rc);
        });
        return t;
    }

    // read binning by two tables (tsx_hip_bin_stats_host): this is A, oOther is B; per record the windows that hit each
    // table, and (pClasses) its class TSX_HIP_BIN_*
    std::vector<tsx_hip_bin_stats> binStats(TSXHashMapHIP &oOther, const char *pText, size_t iBytes, const tsx_hip_bin_rule &oRule,
                                            std::vector<uint8_t> *pClasses = nullptr, size_t iChunkBytes = 0) {
        // a first guess of 256 bytes per record; a text with shorter records is binned again with the exact count
        std::vector<tsx_hip_bin_stats> out(iBytes / 256 + 16);
        std::vector<uint8_t> cls(pClasses ? out.size() : 0);
        size_t n = 0;
        int rc = tsx_hip_bin_stats_host(m_pMap, oOther.m_pMap, pText, iBytes, &oRule, out.data(), pClasses ? cls.data() : nullptr,
                                        out.size(), &n, iChunkBytes);
        if (rc == TSX_HIP_ERANGE) {
            out.resize(n);
            if (pClasses) cls.resize(n);
            rc = tsx_hip_bin_stats_host(m_pMap, oOther.m_pMap, pText, iBytes, &oRule, out.data(), pClasses ? cls.data() : nullptr, n,
                                        &n, iChunkBytes);
        }
        if (rc == TSX_HIP_EINVAL) throw TSXException(tsx_hip_last_error(), rc);   // (the refusal says which argument)
        check(rc);
        out.resize(n);
        if (pClasses) { cls.resize(n); pClasses->swap(cls); }
        return out;
    }
    // tsx_hip_bin_reads_host: the records of the text split by class into sPaths (a, b, ambiguous, none; created /
    // truncated; an empty path counts the class and writes nothing)
    tsx_hip_bin_totals binReads(TSXHashMapHIP &oOther, const char *pText, size_t iBytes, const tsx_hip_bin_rule &oRule,
                                const std::string (&sPaths)[4], size_t iChunkBytes = 0) {
        int fds[4] = {-1, -1, -1, -1};
        for (int i = 0; i < 4; ++i) {
            if (sPaths[i].empty()) continue;
            fds[i] = open(sPaths[i].c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
            if (fds[i] < 0) {
                for (int j = 0; j < i; ++j) if (fds[j] >= 0) close(fds[j]);
                throw TSXException("could not open " + sPaths[i] + " for writing", TSX_HIP_EIO);
            }
        }
        const tsx_hip_bin_io io = {fds[0], fds[1], fds[2], fds[3]};
        tsx_hip_bin_totals oTotals;
        int rc = tsx_hip_bin_reads_host(m_pMap, oOther.m_pMap, pText, iBytes, &oRule, &io, iChunkBytes, &oTotals);
        for (int i = 0; i < 4; ++i)
            if (fds[i] >= 0 && close(fds[i]) != 0 && rc == TSX_HIP_OK) rc = TSX_HIP_EIO;
        if (rc == TSX_HIP_EINVAL) throw TSXException(tsx_hip_last_error(), rc);
        check(rc);
        return oTotals;
    }

    // FASTXreader<FASTAEntry> (FastXReader.h:97-116) reads two lines per record, FASTQEntry (:62-95) four
    void setRecordLines(int iLines) { check(tsx_hip_set_record_lines(m_pMap, iLines)); }
    // canonical counting: a k-mer and its reverse complement share one counter (empty table only)
    void setCanonical(bool bOn) { check(tsx_hip_set_canonical(m_pMap, bOn ? 1 : 0)); }
    // base rule: which windows are k-mers -- only ACGTacgt bytes, every quality byte >= iMinQualChar (0 = off; FASTQ)
    void setBaseRule(bool bAcgtOnly, int iMinQualChar) { check(tsx_hip_set_base_rule(m_pMap, bAcgtOnly ? 1 : 0, iMinQualChar)); }

    // countKMers body (main.cpp:104-218): whole FASTQ text -> table
    void countFastq(const char *pText, size_t iBytes) { check(tsx_hip_count_fastq_host(m_pMap, pText, iBytes)); }
    // the same for a blocked gzip (BGZF) file image: inflated on the device (FastXReader.h:178-206 uses zlib)
    void countFastqBgzf(const void *pGz, size_t iBytes) {
        int rc = tsx_hip_count_fastq_bgzf_host(m_pMap, pGz, iBytes);
        if (rc == TSX_HIP_EINVAL) throw TSXException(std::string("BGZF input: ") + tsx_hip_last_error(), rc);
        check(rc);
    }
    // wrapped (multi-line) FASTA: the sequence lines of a record joined on the device (csrc/tsx_fasta.h), then counted
    // as two-line records -- whatever setRecordLines says, which stays as it is
    void countFasta(const char *pText, size_t iBytes) {
        int rc = tsx_hip_count_fasta_host(m_pMap, pText, iBytes);
        if (rc == TSX_HIP_EINVAL) throw TSXException(std::string("wrapped FASTA input: ") + tsx_hip_last_error(), rc);
        check(rc);
    }
    void countFastaBgzf(const void *pGz, size_t iBytes) {
        int rc = tsx_hip_count_fasta_bgzf_host(m_pMap, pGz, iBytes);
        if (rc == TSX_HIP_EINVAL) throw TSXException(std::string("wrapped FASTA input: ") + tsx_hip_last_error(), rc);
        check(rc);
    }

    // empties the table (the reference has no counterpart: its maps are filled once)
    void clear() { check(tsx_hip_clear(m_pMap)); }

    tsx_hip_stats stats() {
        tsx_hip_stats s;
        check(tsx_hip_get_stats(m_pMap, &s));
        return s;
    }

    // print_stats (TSXHashMap.h:390-395)
    void print_stats() {
        tsx_hip_stats s = stats();
        std::cerr << "Used fields: " << s.distinct << std::endl;
        std::cerr << "Available fields: " << (double)m_oLayout.slots << std::endl;
        std::cerr << "k=" << m_iK << " l=" << (uint32_t)m_iL << " entry limbs=" << m_oLayout.entry_limbs
                  << " storage bits=" << m_oLayout.count_bits << std::endl;
    }

    tsx_hip_map *handle() { return m_pMap; }

private:
    tsx_hip_combine_stats combineInto(tsx_hip_map *pOut, TSXHashMapHIP &oOther, const tsx_hip_combine_rule &oRule) {
        tsx_hip_combine_stats s;
        const int rc = tsx_hip_combine(pOut, m_pMap, oOther.m_pMap, &oRule, &s);
        if (rc == TSX_HIP_EINVAL) throw TSXException(tsx_hip_last_error(), rc);   // (the refusal says which argument)
        check(rc);
        return s;
    }
    static void check(int rc) {
        if (rc == TSX_HIP_OK) return;
        std::string msg = tsx_hip_strerror(rc);
        if (rc == TSX_HIP_EHIP || rc == TSX_HIP_ENODEVICE || rc == TSX_HIP_ENOMEM || rc == TSX_HIP_EIO ||
            rc == TSX_HIP_EFORMAT || rc == TSX_HIP_EPAIR) {
            msg += " (";
            msg += tsx_hip_last_error();
            msg += ")";
        }
        throw TSXException(msg, rc);
    }

    tsx_hip_map *m_pMap = nullptr;
    tsx_hip_layout m_oLayout;
    const uint8_t m_iL;
    const uint32_t m_iK;
    const uint8_t m_iThreads;
};

// The same surface over the GPUs of one node (tsx_hip_group_*, csrc/tsx_multi.cpp): reads shard across the GPUs,
// the per-GPU tables are merged over RCCL, every k-mer then lives on the GPU that owns it.
class TSXHashMapHIPGroup {
public:
    // piDevices: HIP ordinal per rank (nullptr: 0 .. iGpus-1); iComm 0 = RCCL, 1 = device copies (ranks may share a GPU)
    TSXHashMapHIPGroup(int iGpus, const int *piDevices, uint8_t iL, uint32_t iStorageBits, uint16_t iK, uint64_t iHashSeed = 1,
                       int iComm = 0)
        : m_iK(iK) {
        check(tsx_hip_group_create(&m_pGroup, iGpus, piDevices, iK, iL, (int)iStorageBits, 0, iHashSeed, iComm));
        check(tsx_hip_get_layout(tsx_hip_group_map(m_pGroup, 0), &m_oLayout));
        std::cerr << "Creating " << iGpus << " arrays with " << m_oLayout.table_bytes << " bytes for " << m_oLayout.slots
                  << " places each (" << tsx_hip_group_comm_name(m_pGroup) << " merge)." << std::endl;
    }
    ~TSXHashMapHIPGroup() { tsx_hip_group_destroy(m_pGroup); }
    TSXHashMapHIPGroup(const TSXHashMapHIPGroup &) = delete;
    TSXHashMapHIPGroup &operator=(const TSXHashMapHIPGroup &) = delete;

    const tsx_hip_layout &getLayout() const { return m_oLayout; }
    int size() const { return tsx_hip_group_size(m_pGroup); }
    tsx_hip_map *rankMap(int iRank) { return tsx_hip_group_map(m_pGroup, iRank); }
    void setRecordLines(int iLines) { check(tsx_hip_group_set_record_lines(m_pGroup, iLines)); }
    // canonical counting on every GPU's table (the merge only: not with the minimizer exchange)
    void setCanonical(bool bOn) { check(tsx_hip_group_set_canonical(m_pGroup, bOn ? 1 : 0)); }
    // the base rule on every GPU's table (the merge only: not with the minimizer exchange)
    void setBaseRule(bool bAcgtOnly, int iMinQualChar) { check(tsx_hip_group_set_base_rule(m_pGroup, bAcgtOnly ? 1 : 0, iMinQualChar)); }
    // 0: per-GPU tables merged after the count (any k); 1: the minimizer exchange (20 <= k <= 32, at most 16 GPUs)
    void setExchange(int iMode) { check(tsx_hip_group_set_exchange(m_pGroup, iMode)); }
    int exchange() const { return tsx_hip_group_exchange(m_pGroup); }
    void clear() { check(tsx_hip_group_clear(m_pGroup)); }
    // countKMers (main.cpp:104-218) over all GPUs + the merge of the tables
    void countFastq(const char *pText, size_t iBytes) { check(tsx_hip_group_count_fastq_host(m_pGroup, pText, iBytes)); }
    void getKmerCounts(const std::vector<uint64_t> &limbs, size_t n, std::vector<uint64_t> &out) {
        out.resize(n);
        check(tsx_hip_group_get_counts_host(m_pGroup, limbs.data(), n, out.data()));
    }
    tsx_kmer_t fromSequence(const std::string &seq) const {
        tsx_kmer_t out(m_oLayout.key_limbs);
        if (tsx_hip_encode(seq.c_str(), m_iK, out.data()) != TSX_HIP_OK) throw TSXException("bad k-mer", TSX_HIP_EINVAL);
        return out;
    }
    tsx_hip_stats stats() {
        tsx_hip_stats s;
        check(tsx_hip_group_get_stats(m_pGroup, &s));
        return s;
    }
    uint64_t exchangedEntries() const { return tsx_hip_group_exchanged_entries(m_pGroup); }
    uint32_t exchangeRounds() const { return tsx_hip_group_exchange_rounds(m_pGroup); }
    // the histogram / .count file of the whole group (the ranks' tables are disjoint after countFastq)
    std::vector<uint64_t> histogram(size_t iBins) {
        std::vector<uint64_t> h(iBins);
        check(tsx_hip_group_histogram_host(m_pGroup, h.data(), iBins));
        return h;
    }
    uint64_t write_counts(const std::string &sPath, uint64_t iLower = 1, uint64_t iUpper = UINT64_MAX) {
        return tsx_write_counts_file(sPath, [&](int fd, uint64_t *l, uint64_t *b) {
            return tsx_hip_group_write_counts_host(m_pGroup, fd, iLower, iUpper, 0, l, b);
        }, check);
    }
    void print_stats() {
        tsx_hip_stats s = stats();
        std::cerr << "Used fields: " << s.distinct << std::endl;
        std::cerr << "Available fields: " << (double)m_oLayout.slots * size() << std::endl;
        std::cerr << "k=" << m_iK << " l=" << m_oLayout.l << " x " << size() << " GPUs, entry limbs=" << m_oLayout.entry_limbs
                  << " storage bits=" << m_oLayout.count_bits << std::endl;
    }

private:
    static void check(int rc) {
        if (rc == TSX_HIP_OK) return;
        std::string msg = tsx_hip_strerror(rc);
        const std::string why = tsx_hip_group_last_error();
        if (!why.empty()) msg += " (" + why + ")";
        throw TSXException(msg, rc);
    }
    tsx_hip_group *m_pGroup = nullptr;
    tsx_hip_layout m_oLayout;
    const uint32_t m_iK;
};

#endif  // TSXCOUNT_TSXHASHMAPHIP_H
