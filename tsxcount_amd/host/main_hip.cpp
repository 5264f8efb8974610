// main_hip.cpp -- the tsxCount command line (src/mains/main.cpp) with the one
// new mode this repo adds: --mode=HIP.  Options, defaults, console lines and
// the --check procedure follow main.cpp:30-40,404-507 and :222-396; the CPU
// modes stay in the reference build.  cli_options.h holds the options and what
// they refuse; this file runs what is left.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <chrono>
#include <cmath>
#include <fstream>
#include <memory>
#include <unordered_map>

#include "cli_options.h"

// A return code of the C ABI as a TSXException.  The last-error detail is appended always (the calls made with nothing
// but a status to go by) or for the codes that carry one: HIP, IO, NOMEM and, from the pair calls, PAIR.
static void check_rc(int rc, bool always_detail) {
    if (rc == TSX_HIP_OK) return;
    std::string msg = tsx_hip_strerror(rc);
    if (always_detail || rc == TSX_HIP_EHIP || rc == TSX_HIP_EIO || rc == TSX_HIP_ENOMEM || rc == TSX_HIP_EPAIR)
        msg += std::string(" (") + tsx_hip_last_error() + ")";
    throw TSXException(msg, rc);
}
static void check(int rc) { check_rc(rc, false); }

// FastXReader.h:178-206: a .gz input read through zlib (any gzip stream, BGZF included)
static bool read_gz(const std::string &path, std::vector<char> &owned) {
    gzFile f = gzopen(path.c_str(), "rb");
    if (!f) return false;
    static char buf[1 << 16];
    int r;
    while ((r = gzread(f, buf, sizeof buf)) > 0) owned.insert(owned.end(), buf, buf + r);
    gzclose(f);
    return r == 0;
}

// One input, whole and in memory: a plain file is mmap'ed; .gz (FastXReader.h:178-206 picks zlib mode by the same suffix
// test): a blocked gzip file (BGZF) is mmap'ed as it is, to be inflated on the GPU (bgzf = true), any other gzip stream
// goes through zlib here.  The mapping is released with the object.
struct input_text {
    std::vector<char> owned;
    const char *data = nullptr;
    size_t n = 0;
    void *map = nullptr;
    bool bgzf = false;
    input_text() = default;
    input_text(const input_text &) = delete;
    input_text &operator=(const input_text &) = delete;
    ~input_text() { release(); }
    void release() {
        if (map) munmap(map, n);
        map = nullptr;
    }
    // says "Could not read" and returns false where the file cannot be read
    bool load(const std::string &path, bool allow_bgzf) {
        if (load_input(path, allow_bgzf)) return true;
        std::cerr << "Could not read " << path << std::endl;
        return false;
    }
    // a BGZF file becomes its text, inflated on the device (what reads records takes text; the counts take BGZF as it is)
    void inflate_on_device(int device, bool always_detail) {
        if (!bgzf) return;
        size_t members = 0, tb = 0, got = 0;
        check_rc(tsx_hip_bgzf_index_host(data, n, &members, &tb), always_detail);
        std::vector<char> inflated(tb ? tb : 1);
        check_rc(tsx_hip_inflate_bgzf_host(device, data, n, inflated.data(), tb, &got), always_detail);
        inflated.resize(got);
        take(inflated);
    }
    // the device path of a BGZF count needs two batch-sized text buffers next to the table: without them (e is that
    // ENOMEM) the input is read the way the reference reads it, zlib on the host, and goes on as plain text
    bool fall_back_to_zlib(const std::string &path, const TSXException &e) {
        std::cerr << "BGZF on the device: " << e.what() << " -- reading through zlib instead" << std::endl;
        std::vector<char> inflated;
        if (!read_gz(path, inflated)) {
            std::cerr << "Could not read " << path << std::endl;
            return false;
        }
        take(inflated);
        return true;
    }

private:
    void take(std::vector<char> &plain) {
        release();
        owned.swap(plain);
        data = owned.data();
        n = owned.size();
        bgzf = false;
    }
    bool load_input(const std::string &path, bool allow_bgzf) {
        if (path.size() > 3 && path.rfind(".gz") == path.size() - 3) {
            int zfd = open(path.c_str(), O_RDONLY);
            struct stat zst;
            if (allow_bgzf && zfd >= 0 && fstat(zfd, &zst) == 0 && zst.st_size > 0) {
                void *zm = mmap(nullptr, (size_t)zst.st_size, PROT_READ, MAP_PRIVATE, zfd, 0);
                if (zm != MAP_FAILED) {
                    size_t members = 0, tb = 0;
                    if (tsx_hip_bgzf_index_host(zm, (size_t)zst.st_size, &members, &tb) == TSX_HIP_OK) {
                        close(zfd);
                        std::cerr << "Input is BGZF: " << members << " members, " << tb << " bytes of text, inflated on the device"
                                  << std::endl;
                        map = zm; data = (const char *)zm; n = (size_t)zst.st_size; bgzf = true;
                        return true;
                    }
                    munmap(zm, (size_t)zst.st_size);
                }
            }
            if (zfd >= 0) close(zfd);
            const bool ok = read_gz(path, owned);
            data = owned.data(); n = owned.size();
            return ok;
        }
        int fd = open(path.c_str(), O_RDONLY);
        if (fd < 0) return false;
        struct stat st;
        if (fstat(fd, &st) != 0) { close(fd); return false; }
        n = (size_t)st.st_size;
        if (n == 0) { close(fd); data = ""; return true; }
        map = mmap(nullptr, n, PROT_READ, MAP_PRIVATE, fd, 0);
        close(fd);
        if (map == MAP_FAILED) { map = nullptr; return false; }
        data = (const char *)map;
        return true;
    }
};

// The reads of a read call (--filter, --trim, --bin-*, the paired forms): loaded as the counted input is, a BGZF file
// inflated on the device.
static bool load_reads(input_text &in, const std::string &path, const arguments &a, bool always_detail = false) {
    if (!in.load(path, true)) return false;
    in.inflate_on_device(a.device, always_detail);
    return true;
}
// (--format=fasta-wrapped names the format of --input only: the file of a read call goes by its name)
static int record_lines(const std::string &path, const arguments &a) {
    return is_fasta_path(path, is_wrapped(a) ? std::string() : a.format) ? 2 : 4;
}

// canonical counting, the base rule and two-line records, on a table, the probe or a group as it is created
template <typename Map>
static void apply_counting_mode(Map &oMap, const arguments &a) {
    if (is_fasta(a)) oMap.setRecordLines(2);
    if (a.canonical) oMap.setCanonical(true);
    if (a.acgt_only || a.min_qual_char) oMap.setBaseRule(a.acgt_only, a.min_qual_char);
}

static tsx_hip_filter_rule make_filter_rule(const arguments &a) {
    tsx_hip_filter_rule rule;
    rule.lower = a.filter_lower;
    rule.upper = a.filter_upper;
    rule.min_in_range = a.filter_min;
    rule.fraction_ppm = (uint32_t)std::llround(a.filter_fraction * 1e6);
    rule.invert = a.filter_invert ? 1 : 0;
    return rule;
}
static tsx_hip_trim_rule make_trim_rule(const arguments &a) {
    tsx_hip_trim_rule rule;
    rule.lower = a.trim_lower;
    rule.upper = a.trim_upper;
    rule.min_len = a.trim_min_len;
    rule.mode = a.trim_mode == "prefix" ? TSX_HIP_TRIM_PREFIX : TSX_HIP_TRIM_LONGEST;
    rule.reserved = 0;
    return rule;
}

// a file written through a stream: body(f) writes it, and a file that did not close clean is an IO error
template <typename Body>
static void write_file(const std::string &path, Body body) {
    std::ofstream f(path);
    body(f);
    f.close();
    if (!f) throw TSXException("could not write " + path, TSX_HIP_EIO);
}

// an nr x nc matrix of counts: "sparse" writes row<TAB>column<TAB>count for every cell that is not 0, "matrix" a comment
// line and the nr lines of nc numbers
static void write_count_matrix(const std::string &path, const std::vector<uint64_t> &m, size_t nr, size_t nc, const std::string &format,
                               const char *rows, const char *columns) {
    write_file(path, [&](std::ofstream &f) {
        const bool matrix = format == "matrix";
        if (matrix) f << "# rows: " << rows << " 0.." << nr - 1 << ", columns: " << columns << "\n";
        for (size_t i = 0; i < nr; ++i) {
            for (size_t j = 0; j < nc; ++j) {
                const uint64_t n = m[i * nc + j];
                if (matrix) f << n << (j + 1 < nc ? '\t' : '\n');
                else if (n) f << i << '\t' << j << '\t' << n << '\n';
            }
        }
    });
}

// reverse complement of an ACGT string (what --canonical --check pairs up)
static std::string revcomp(const std::string &s) {
    std::string r(s.rbegin(), s.rend());
    for (char &c : r) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : c;
    return r;
}

// --het-histo and --het-pairs: the heterozygous pairs of the table as files, and their totals on stdout
static void write_het(TSXHashMapHIP &oMap, const arguments &a) {
    if (!wants_het(a)) return;
    const tsx_hip_het_rule oRule = {a.het_lower, a.het_upper, a.het_mode == "all" ? TSX_HIP_HET_ALL : TSX_HIP_HET_UNIQUE, 0};
    const size_t nb = (size_t)a.het_max + 2;
    std::vector<uint64_t> m;
    const tsx_hip_het_stats s = oMap.hetHistogram(oRule, nb, nb, m);
    if (!a.het_histo.empty()) {
        write_count_matrix(a.het_histo, m, nb, nb, a.het_format, "minor count", "major count");
        std::cerr << "Wrote the het pair histogram to " << a.het_histo << std::endl;
    }
    if (!a.het_pairs.empty()) {
        const uint64_t iPairs = oMap.writeHetPairs(a.het_pairs, oRule);
        std::cerr << "Wrote " << iPairs << " het pairs to " << a.het_pairs << std::endl;
    }
    std::cout << "het\t" << s.kmers_in_range << '\t' << s.paired << '\t' << s.pairs << '\t' << s.families_2 << '\t'
              << s.families_3plus << std::endl;
}
static void write_het(TSXHashMapHIPGroup &, const arguments &a) {   // (main refuses --gpus > 1 and runs --gpus=1 on the one table)
    if (wants_het(a))
        throw TSXException("--het-histo and --het-pairs need the one table of a one-GPU run, not a group", TSX_HIP_EINVAL);
}

// --output and --histo, for one table or a group of them (after the count and the check)
template <typename Map>
static void write_outputs(Map &oMap, const arguments &a) {
    if (!a.output.empty()) {
        const uint64_t iLines = oMap.write_counts(a.output, a.lower, a.upper);
        std::cerr << "Wrote " << iLines << " kmers to " << a.output << std::endl;
    }
    if (!a.histo.empty()) {
        const std::vector<uint64_t> h = oMap.histogram((size_t)a.histo_max + 2);
        write_file(a.histo, [&](std::ofstream &f) {
            for (uint64_t c = 1; c <= a.histo_max; ++c)
                if (h[c]) f << c << '\t' << h[c] << '\n';
            f << a.histo_max + 1 << '\t' << h[a.histo_max + 1] << '\n';
        });
        std::cerr << "Wrote the count histogram to " << a.histo << std::endl;
    }
}

// --filter / --trim over mate pairs: two files or one interleaved file, where the single-end forms run.
static int run_pairs(tsx_hip_map *pMap, const arguments &a, bool trim) {
    const std::vector<std::string> in = split_commas(trim ? a.trim_input : a.filter_input);
    const std::vector<std::string> out = split_commas(trim ? a.trim : a.filter);
    const std::string &singles = trim ? a.trim_singles : a.filter_singles;
    const std::vector<std::string> sg = singles.empty() ? std::vector<std::string>() : split_commas(singles);
    const bool inter = in.size() == 1;
    input_text t1, t2;
    if (!load_reads(t1, in[0], a) || (!inter && !load_reads(t2, in[1], a))) return 3;
    const int lines = record_lines(in[0], a);
    if (!inter && lines != record_lines(in[1], a)) {
        std::cerr << "paired input: " << in[0] << " and " << in[1] << " differ in format" << std::endl;
        return 3;
    }
    check(tsx_hip_set_record_lines(pMap, lines));
    const std::string paths[4] = {out[0], inter ? std::string() : out[1], sg.empty() ? std::string() : sg[0],
                                  sg.size() > 1 ? sg[1] : std::string()};
    tsx_hip_pair_totals t;
    if (trim) {
        t = tsx_trim_pairs(pMap, t1.data, t1.n, inter ? nullptr : t2.data, t2.n, make_trim_rule(a), a.pair_names, paths, 0, check);
        std::cout << "pairs\t" << t.pairs << '\t' << t.kept << '\t' << t.single1 << '\t' << t.single2 << '\t' << t.bases_in << '\t'
                  << t.bases_kept << std::endl;
    } else {
        t = tsx_filter_pairs(pMap, t1.data, t1.n, inter ? nullptr : t2.data, t2.n, make_filter_rule(a),
                             a.filter_pairs == "any" ? TSX_HIP_PAIR_ANY : TSX_HIP_PAIR_BOTH, a.pair_names, paths, 0, check);
        std::cout << "pairs\t" << t.pairs << '\t' << t.kept << '\t' << t.single1 << '\t' << t.single2 << std::endl;
    }
    std::cerr << "Wrote " << t.kept << " of " << t.pairs << " pairs (" << t.bytes1 + t.bytes2 << " bytes), " << t.single1 << " + "
              << t.single2 << " single mates" << std::endl;
    return 0;
}

// --filter, --read-stats and --read-medians on one table, after the count, the check and --output / --histo.
static int run_read_queries(tsx_hip_map *pMap, const arguments &a) {
    const std::string path = a.filter_input.empty() ? a.input_path : a.filter_input;
    input_text in;
    if (!load_reads(in, path, a)) return 3;
    check(tsx_hip_set_record_lines(pMap, record_lines(path, a)));
    if (!a.read_stats.empty()) {
        const std::vector<tsx_hip_read_stats> st = tsx_query_reads(pMap, in.data, in.n, a.filter_lower, a.filter_upper, 0, check);
        write_file(a.read_stats, [&](std::ofstream &f) {
            for (size_t i = 0; i < st.size(); ++i)
                f << i << '\t' << st[i].kmers << '\t' << st[i].in_range << '\t' << st[i].min_count << '\t' << st[i].sum_count << '\n';
        });
        std::cerr << "Wrote the k-mer stats of " << st.size() << " records to " << a.read_stats << std::endl;
    }
    if (!a.read_medians.empty()) {
        const std::vector<tsx_hip_read_median> md = tsx_median_reads(pMap, in.data, in.n, 0, check);
        write_file(a.read_medians, [&](std::ofstream &f) {
            for (size_t i = 0; i < md.size(); ++i) f << i << '\t' << md[i].kmers << '\t' << md[i].median << '\n';
        });
        std::cerr << "Wrote the median k-mer counts of " << md.size() << " records to " << a.read_medians << std::endl;
    }
    if (!a.filter.empty()) {
        std::pair<uint64_t, uint64_t> r;
        if (a.filter_median) {
            tsx_hip_median_rule rule;
            rule.lower = a.filter_median_lower;
            rule.upper = a.filter_median_upper;
            rule.invert = a.filter_invert ? 1 : 0;
            rule.reserved = 0;
            r = tsx_filter_median(pMap, in.data, in.n, rule, a.filter, 0, check);
        } else {
            r = tsx_filter_reads(pMap, in.data, in.n, make_filter_rule(a), a.filter, 0, check);
        }
        std::cerr << "Wrote " << r.first << " records (" << r.second << " bytes) to " << a.filter << std::endl;
    }
    return 0;
}

// --trim and --trim-spans on one table, where --filter runs.
static int run_trim(tsx_hip_map *pMap, const arguments &a) {
    const std::string path = a.trim_input.empty() ? a.input_path : a.trim_input;
    input_text in;
    if (!load_reads(in, path, a)) return 3;
    check(tsx_hip_set_record_lines(pMap, record_lines(path, a)));
    const tsx_hip_trim_rule rule = make_trim_rule(a);
    if (!a.trim_spans.empty()) {
        const std::vector<tsx_hip_trim_span> sp = tsx_trim_spans(pMap, in.data, in.n, rule, 0, check);
        write_file(a.trim_spans, [&](std::ofstream &f) {
            for (size_t i = 0; i < sp.size(); ++i) f << i << '\t' << sp[i].start << '\t' << sp[i].length << '\n';
        });
        std::cerr << "Wrote the kept spans of " << sp.size() << " records to " << a.trim_spans << std::endl;
    }
    if (!a.trim.empty()) {
        const tsx_hip_trim_totals t = tsx_trim_reads(pMap, in.data, in.n, rule, a.trim, 0, check);
        std::cout << "trim\t" << t.records << '\t' << t.kept << '\t' << t.bases_in << '\t' << t.bases_kept << std::endl;
        std::cerr << "Wrote " << t.kept << " trimmed records (" << t.bytes << " bytes) to " << a.trim << std::endl;
    }
    return 0;
}

// what ends a run on one table, behind the count, the check, the outputs and the set operation: the read queries, then
// the trim, on the table that stands now; rc is what the check found
static int finish(tsx_hip_map *pMap, int rc, const arguments &a) {
    const int rq = !wants_queries(a) ? 0 : filter_paired(a) ? run_pairs(pMap, a, false) : run_read_queries(pMap, a);
    const int rt = !wants_trim(a) ? 0 : trim_paired(a) ? run_pairs(pMap, a, true) : run_trim(pMap, a);
    return rc ? rc : rq ? rq : rt;
}

// --save, after the count and the check (one table only: a group refuses it earlier)
static void save_database(TSXHashMapHIP &oMap, const arguments &a) {
    if (a.save.empty()) return;
    const uint64_t iEntries = oMap.saveDatabase(a.save);
    std::cerr << "Wrote a k-mer database of " << iEntries << " kmers to " << a.save << std::endl;
}
static void save_database(TSXHashMapHIPGroup &, const arguments &) {}

// --joint-histo: the joint spectrum of A and B as a file, and its three sums on stdout
static void write_joint(TSXHashMapHIP &oA, TSXHashMapHIP &oB, const arguments &a) {
    const size_t na = (size_t)a.joint_max_a + 2, nb = (size_t)a.joint_max_b + 2;
    std::vector<uint64_t> m;
    oA.jointHistogram(oB, na, nb, m);
    uint64_t a_only = 0, b_only = 0, both = 0;
    for (size_t i = 0; i < na; ++i)
        for (size_t j = 0; j < nb; ++j) (i == 0 ? b_only : j == 0 ? a_only : both) += m[i * nb + j];
    write_count_matrix(a.joint_histo, m, na, nb, a.joint_format, "count in A", "count in B");
    std::cout << "joint\t" << a_only << '\t' << b_only << '\t' << both << std::endl;
    std::cerr << "Wrote the joint histogram to " << a.joint_histo << std::endl;
}

// --bin-*: the records of --bin-input by the table they hit more, where --compare and --joint-histo run
static int run_bin(TSXHashMapHIP &oA, TSXHashMapHIP &oB, const arguments &a) {
    const std::string path = a.bin_input.empty() ? a.input_path : a.bin_input;
    input_text in;
    if (!load_reads(in, path, a, true)) return 3;
    oA.setRecordLines(record_lines(path, a));
    const tsx_hip_bin_rule rule = {a.a_lower, a.a_upper, a.b_lower, a.b_upper, a.bin_min_hits, a.bin_ratio_milli, 0};
    static const char *const names[4] = {"a", "b", "ambiguous", "none"};
    uint64_t records = 0, n[4] = {0, 0, 0, 0};
    if (!a.bin_stats.empty()) {
        std::vector<uint8_t> cls;
        const std::vector<tsx_hip_bin_stats> st = oA.binStats(oB, in.data, in.n, rule, &cls);
        write_file(a.bin_stats, [&](std::ofstream &f) {
            for (size_t i = 0; i < st.size(); ++i) {
                f << i << '\t' << st[i].kmers << '\t' << st[i].hits_a << '\t' << st[i].hits_b << '\t' << st[i].hits_both << '\t'
                  << names[cls[i] & 3] << '\n';
                ++n[cls[i] & 3];
            }
        });
        records = st.size();
        std::cerr << "Wrote the bin stats of " << st.size() << " records to " << a.bin_stats << std::endl;
    }
    if (wants_bin_reads(a)) {
        const std::string paths[4] = {a.bin_a, a.bin_b, a.bin_ambiguous, a.bin_none};
        const tsx_hip_bin_totals bt = oA.binReads(oB, in.data, in.n, rule, paths);
        records = bt.records;
        for (int c = 0; c < 4; ++c) {
            n[c] = bt.n[c];
            if (!paths[c].empty())
                std::cerr << "Wrote " << bt.n[c] << " records (" << bt.bytes[c] << " bytes) to " << paths[c] << std::endl;
        }
    }
    std::cout << "bin\t" << records << '\t' << n[0] << '\t' << n[1] << '\t' << n[2] << '\t' << n[3] << std::endl;
    return 0;
}

// --l=auto and --estimate: the input is sketched on a minimal probe map that carries its counting mode, the estimate of
// its distinct k-mers picks l (a.l, for the count that follows), and one line says so:
// estimate<TAB>kmers<TAB>distinct<TAB>l<TAB>load.
static void size_table(arguments &a, const input_text &in) {
    std::vector<uint8_t> regs;
    tsx_hip_sketch_totals t;
    // the probe map: the smallest l that has a layout (4; a long k-mer needs its func bits to fit four limbs: k = 127, l >= 11)
    const int l_hi = std::min(36, 2 * a.k - 1);
    int l_min = std::min(4, l_hi);
    std::unique_ptr<TSXHashMapHIP> pProbe;
    while (!pProbe) {
        try {
            pProbe.reset(new TSXHashMapHIP((uint8_t)l_min, (uint32_t)a.storagebits, (uint16_t)a.k, (uint8_t)a.threads, a.seed, a.device, 0));
        } catch (const TSXException &e) {
            if (e.code() != TSX_HIP_EINVAL || l_min >= l_hi) throw;
            ++l_min;
        }
    }
    apply_counting_mode(*pProbe, a);
    t = in.bgzf ? pProbe->sketchKmersBgzf(in.data, in.n, regs) : pProbe->sketchKmers(in.data, in.n, regs);
    pProbe.reset();
    const double distinct = TSXHashMapHIP::estimate(regs);
    bool clamped = false;
    a.l = std::max(l_min, TSXHashMapHIP::suggestL(a.k, distinct, a.load_factor, 14, &clamped));
    const double load = distinct / std::ldexp(1.0, a.l);
    char line[160];
    snprintf(line, sizeof line, "estimate\t%llu\t%.0f\t%d\t%.3f", (unsigned long long)t.kmers, distinct, a.l, load);
    std::cout << line << std::endl;
    std::cerr << "Table sizing: about " << (unsigned long long)std::llround(distinct) << " distinct k-mers among " << t.kmers
              << ", l=" << a.l << " (expected load " << load << ")" << std::endl;
    if (clamped)
        std::cerr << "Warning: l cannot exceed " << a.l << " for k=" << a.k << ": the expected load " << load
                  << " is above 0.9, the count may end with a full table" << std::endl;
}

// "Added a total of ..." and the --check of main.cpp:224-396, for one table or a group of them
template <typename Map>
static int report_and_check(Map &oMap, const arguments &a, double dt, bool outputs = true) {
    tsx_hip_stats st = oMap.stats();
    std::cout << "Added a total of " << st.distinct << " different kmers" << std::endl;
    std::cerr << "add calls: " << st.kmers_added << std::endl;
    std::cerr << "count time [s]: " << dt << " (" << (dt > 0 ? st.kmers_added / dt : 0) << " k-mers/s, host to table)"
              << std::endl;
    int rc = 0;
    if (a.check) {  // main.cpp:224-396
        std::string sRefFilename = a.input_path + "." + std::to_string(a.k) + ".count";
        std::cout << "Checking kmer counts against manual hashmap ..." << std::endl;
        std::cerr << "Loading reference file: " << sRefFilename << std::endl;
        std::ifstream file(sRefFilename);
        if (!file.is_open()) {
            std::cerr << "Could not open " << sRefFilename << std::endl;
            return 4;
        }
        std::vector<uint64_t> limbs, expect, got;
        std::vector<std::string> names;
        std::string line;
        uint64_t iRefCount = 0, totalerrors = 0;
        // --canonical: the file holds forward counts f; a listed k-mer x must count f(x) + f(rc x) (f(x) for a
        // palindrome), and the table holds one entry per strand pair
        std::unordered_map<std::string, uint64_t> fwd;
        uint64_t iPairs = 0;
        if (a.canonical) {
            while (std::getline(file, line)) {
                const size_t tab = line.find('\t');
                if (tab == std::string::npos || (int)tab != a.k) continue;
                fwd[line.substr(0, tab)] = strtoull(line.c_str() + tab + 1, nullptr, 10);
            }
            file.clear();
            file.seekg(0);
        }
        auto flush = [&]() {
            if (expect.empty()) return;
            oMap.getKmerCounts(limbs, expect.size(), got);
            for (size_t i = 0; i < expect.size(); ++i)
                if (got[i] != expect[i]) {
                    ++totalerrors;
                    if (totalerrors <= 20)
                        std::cout << "kmer: ( " << names[i] << " ): " << got[i] << " Should be " << expect[i] << std::endl;
                    if (a.checkabort) exit(200);  // main.cpp:285-291
                }
            std::cout << "Checked " << expect.size() << " kmers" << std::endl;
            iRefCount += expect.size();
            limbs.clear(); expect.clear(); names.clear();
        };
        while (std::getline(file, line)) {
            size_t tab = line.find('\t');
            if (tab == std::string::npos) continue;
            std::string kmer = line.substr(0, tab);
            if ((int)kmer.size() != a.k) continue;
            tsx_kmer_t enc = oMap.fromSequence(kmer);
            limbs.insert(limbs.end(), enc.begin(), enc.end());
            uint64_t want = strtoull(line.c_str() + tab + 1, nullptr, 10);
            if (a.canonical) {
                const std::string rc = revcomp(kmer);
                const auto it = fwd.find(rc);
                if (rc != kmer && it != fwd.end()) want += it->second;
                if (rc >= kmer || it == fwd.end()) ++iPairs;   // the pair is counted once: at its smaller listed strand
            }
            expect.push_back(want);
            names.push_back(kmer);
            if (expect.size() >= 100000) flush();  // main.cpp:263
        }
        flush();
        std::cout << "total errors" << totalerrors << std::endl;
        std::cout << "Kmer count check completed." << std::endl;
        if (a.canonical) iRefCount = iPairs;
        std::cout << "Reference kmer count: " << iRefCount << (a.canonical ? " (strand pairs)" : "") << std::endl;
        std::cout << "tsxCount kmer count: " << st.distinct << std::endl;
        if (totalerrors || iRefCount != st.distinct) rc = 5;
    }
    if (outputs) {   // (after a set operation its result is saved and written instead)
        save_database(oMap, a);
        write_outputs(oMap, a);
    }
    write_het(oMap, a);   // (of the table as it is now, whatever --op makes of it later)
    oMap.print_stats();
    return rc;
}

// --gpus N: one table per GPU, the text cut into N shards of whole records, the tables merged over RCCL
// (tsx_hip_group_*); --check asks every k-mer of the GPU that owns it
static int run_group(const arguments &a) {
    std::cerr << "Creating TSXHashMap HIP on " << a.gpus << " GPUs" << std::endl;
    TSXHashMapHIPGroup oGroup(a.gpus, a.devices.empty() ? nullptr : a.devices.data(), (uint8_t)a.l, (uint32_t)a.storagebits,
                              (uint16_t)a.k, a.seed, a.comm == "copy" ? 1 : 0);
    if (is_fasta(a)) std::cerr << "Format=FASTA (2 lines per record)" << std::endl;
    apply_counting_mode(oGroup, a);
    // the minimizer exchange where it applies (auto: from 4 GPUs on, as bench.py, and not with --canonical); --exchange=mini
    // insists on it
    const bool rule = a.acgt_only || a.min_qual_char;
    if (a.exchange == "mini" || (a.exchange == "auto" && !a.canonical && !rule && a.gpus >= 4 && a.gpus <= 16 && a.k >= 20 && a.k <= 32)) {
        try { oGroup.setExchange(1); }
        catch (const TSXException &e) { if (a.exchange == "mini") throw; }
    }
    std::cerr << "exchange: " << (oGroup.exchange() == 1 ? "minimizer owners (strip descriptions travel, nothing is merged)" : "per-GPU tables merged") << std::endl;
    input_text in;
    // (.gz: inflated by zlib on the host, as the reference's reader does -- the record cuts need the text)
    if (!in.load(a.input_path, false)) return 3;
    auto t0 = std::chrono::steady_clock::now();
    oGroup.countFastq(in.data, in.n);
    double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    in.release();
    std::cerr << (oGroup.exchange() == 1 ? "descriptions moved between GPUs by the last share: " : "entries moved between GPUs by the merge: ") << oGroup.exchangedEntries();
    if (oGroup.exchange() == 1) std::cerr << " (exchange rounds: " << oGroup.exchangeRounds() << ")";
    std::cerr << std::endl;
    const int rc = report_and_check(oGroup, a, dt);
    if (!wants_queries(a)) return rc;
    const int rq = run_read_queries(oGroup.rankMap(0), a);   // one GPU: its table holds every k-mer
    return rc ? rc : rq;
}

// --min-count=2, pass 1: the input into the prefilter (the count that follows is pass 2); false when the input could
// not be read again
static bool prefilter_pass(TSXHashMapHIP &oMap, const arguments &a, input_text &in) {
    const int bits = a.prefilter_bits ? a.prefilter_bits : std::min(38, std::max(12, a.l + 6));
    if (in.bgzf) {
        try {
            oMap.prefilterBgzf(in.data, in.n, bits);
        } catch (const TSXException &e) {
            if (e.code() != TSX_HIP_ENOMEM) throw;
            if (!in.fall_back_to_zlib(a.input_path, e)) return false;
        }
    }
    if (!in.bgzf) oMap.prefilter(in.data, in.n, bits);
    oMap.armPrefilter(true);
    return true;
}

// The input into the table: by normalization, or the plain count of FASTQ / two-line FASTA / wrapped FASTA, from text or
// from BGZF as it is; false when the input could not be read again.
static bool count_input(TSXHashMapHIP &oMap, const arguments &a, input_text &in) {
    const bool wrapped = is_wrapped(a);
    if (a.input_path.empty()) return true;   // nothing to count: the loaded tables are the result
    if (!a.normalize.empty()) {
        in.inflate_on_device(a.device, true);   // as the read queries read a BGZF file
        const tsx_hip_normalize_totals nt = oMap.normalizeReads(in.data, in.n, a.normalize_cutoff, a.normalize_round, a.normalize);
        std::cout << "normalize\t" << nt.records << '\t' << nt.kept << '\t' << nt.kmers_seen << '\t' << nt.kmers_added << '\t'
                  << nt.rounds << std::endl;
        std::cerr << "Normalization kept " << nt.kept << " of " << nt.records << " records (cutoff " << a.normalize_cutoff
                  << ", rounds of " << a.normalize_round << ") in " << a.normalize << std::endl;
        return true;
    }
    if (in.bgzf) {
        try {
            if (wrapped) oMap.countFastaBgzf(in.data, in.n);
            else oMap.countFastqBgzf(in.data, in.n);
            return true;
        } catch (const TSXException &e) {
            if (e.code() != TSX_HIP_ENOMEM) throw;
            if (!in.fall_back_to_zlib(a.input_path, e)) return false;
            oMap.clear();   // and counted again from the start, through the staged host path
            for (const std::string &db : a.load) oMap.loadDatabase(db);
        }
    }
    if (wrapped) oMap.countFasta(in.data, in.n);
    else oMap.countFastq(in.data, in.n);
    return true;
}

// --with: B is built like its first database, OUT like A; the result of --op takes A's place from there on
static int run_with(TSXHashMapHIP &oMap, const arguments &a, const db_headers &h, double dt) {
    const int rc = report_and_check(oMap, a, dt, a.op.empty());
    std::cerr << "Creating the second table" << std::endl;
    TSXHashMapHIP oWith((uint8_t)h.with_first.l, (uint32_t)h.with_first.count_bits, (uint16_t)a.k, (uint8_t)a.threads,
                        h.with_first.hash_seed, a.device, h.with_first.overflow_l);
    apply_counting_mode(oWith, a);
    for (const std::string &db : a.with) {
        const uint64_t iEntries = oWith.loadDatabase(db);
        std::cerr << "Loaded " << iEntries << " kmers from " << db << std::endl;
    }
    if (a.compare) {
        const tsx_hip_combine_stats s = oMap.compare(oWith, a.a_lower, a.a_upper, a.b_lower, a.b_upper);
        std::cout << "compare\t" << s.a_in_range << '\t' << s.b_in_range << '\t' << s.both << '\t'
                  << TSXHashMapHIP::jaccard(s) << std::endl;
        std::cout << "compare-sums\t" << s.a_sum_both << '\t' << s.b_sum_both << std::endl;
    }
    if (!a.joint_histo.empty()) write_joint(oMap, oWith, a);
    const int rb = wants_bin(a) ? run_bin(oMap, oWith, a) : 0;
    if (rb) return rc ? rc : rb;
    if (a.op.empty()) return finish(oMap.handle(), rc, a);
    std::cerr << "Creating the result table" << std::endl;
    TSXHashMapHIP oOut((uint8_t)a.l, (uint32_t)a.storagebits, (uint16_t)a.k, (uint8_t)a.threads, a.seed, a.device, h.overflow_l);
    apply_counting_mode(oOut, a);
    const tsx_hip_combine_rule oRule = {op_index(a.op), count_index(a.op_count), a.a_lower, a.a_upper, a.b_lower, a.b_upper};
    const tsx_hip_combine_stats s = oMap.combine(oWith, oOut, oRule);
    std::cout << a.op << ": " << s.out_entries << " different kmers, count sum " << s.out_count_sum << " (first table "
              << s.a_in_range << ", second " << s.b_in_range << ", both " << s.both << " in range)" << std::endl;
    save_database(oOut, a);
    write_outputs(oOut, a);
    return finish(oOut.handle(), rc, a);
}

// one table on one GPU: sized, filled from --load and --input, reported and checked, then what reads it
static int run_one_table(arguments &a, const db_headers &h) {
    input_text in;
    const bool sized = a.l_auto || a.estimate;
    if (sized) {   // the text is loaded once: the count below takes it as it is
        if (!in.load(a.input_path, true)) return 3;
        size_table(a, in);
        if (a.estimate) return 0;
    }
    std::cerr << "Creating TSXHashMap HIP" << std::endl;
    TSXHashMapHIP oMap((uint8_t)a.l, (uint32_t)a.storagebits, (uint16_t)a.k, (uint8_t)a.threads, a.seed, a.device, h.overflow_l);
    if (is_wrapped(a)) std::cerr << "Format=FASTA (wrapped, lines joined)" << std::endl;
    else if (is_fasta(a)) std::cerr << "Format=FASTA (2 lines per record)" << std::endl;
    apply_counting_mode(oMap, a);
    if (!sized && !a.input_path.empty() && !in.load(a.input_path, true)) return 3;
    auto t0 = std::chrono::steady_clock::now();
    for (const std::string &db : a.load) {
        const uint64_t iEntries = oMap.loadDatabase(db);
        std::cerr << "Loaded " << iEntries << " kmers from " << db << std::endl;
    }
    if (a.min_count == 2 && !prefilter_pass(oMap, a, in)) return 3;
    if (!count_input(oMap, a, in)) return 3;
    double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    in.release();
    if (a.min_count == 2) {
        oMap.armPrefilter(false);
        const tsx_hip_prefilter_totals pt = oMap.prefilterStats();
        std::cout << "prefilter\t" << pt.bits << '\t' << pt.seen << '\t' << pt.seen_again << '\t' << pt.admitted << '\t' << pt.skipped << std::endl;
        std::cerr << "Prefilter: " << pt.skipped << " of " << pt.seen << " k-mer occurrences kept out of the table; filter fill "
                  << pt.set_bits_a << " / 2^" << pt.bits << " and " << pt.set_bits_b << " / 2^" << (pt.bits - 2) << " bits" << std::endl;
    }
    if (!a.with.empty()) return run_with(oMap, a, h, dt);
    const int rc = report_and_check(oMap, a, dt);
    return finish(oMap.handle(), rc, a);
}

int main(int argc, char *argv[]) {
    arguments a;
    db_headers h;
    refusal r = parse_options(argc, argv, a);
    if (!r) r = first_refusal(REFUSE_FROM_OPTIONS, a);
    if (!r) r = read_headers(false, a, h);
    if (!r) r = first_refusal(REFUSE_OF_TABLES, a);
    if (!r) r = read_headers(true, a, h);
    if (r) return report(r);
    print_banner(a);
    r = first_refusal(REFUSE_BEHIND_BANNER, a);
    if (r) return report(r);
    try {
        return uses_group(a) ? run_group(a) : run_one_table(a, h);
    } catch (const TSXException &e) {
        std::cerr << "TSXException: " << e.what() << std::endl;
        return e.code() == TSX_HIP_EFULL ? 42 : 10;  // exit(42): TSXHashMap.h:340-343
    }
}
