// main_hip.cpp -- the tsxCount command line (src/mains/main.cpp) with the one
// new mode this repo adds: --mode=HIP.  Options, defaults, console lines and
// the --check procedure follow main.cpp:30-40,404-507 and :222-396; the CPU
// modes stay in the reference build.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "TSXHashMapHIP.h"

struct arguments {
    int k = 14, l = 26, storagebits = 4, threads = 0;  // main.cpp:410-413
    std::string input_path, mode = "HIP", format;   // format: "", "fastq", "fasta" or "fasta-wrapped" ("" = by file name)
    bool check = false, checkabort = false;
    unsigned long long seed = 1;
    int device = 0;
    bool group = false;           // --gpus given: the group path, even for one GPU (its merge then runs through RCCL with one rank)
    int gpus = 1;                 // --gpus N: reads shard across N GPUs, per-GPU tables merged over RCCL
    std::string comm = "rccl";    // --comm=rccl|copy (copy: device-to-device copies, ranks may share a GPU)
    std::string exchange = "auto"; // --exchange=merge|mini|auto: tables merged after the count / minimizer exchange (20 <= k <= 32;
                                  // auto: from 4 GPUs on where it applies)
    std::vector<int> devices;     // --devices=a,b,...: HIP ordinal per rank (default 0 .. N-1)
    bool canonical = false;       // --canonical: a k-mer and its reverse complement share one counter
    bool acgt_only = false;       // --acgt-only: windows with a byte outside ACGTacgt are not k-mers
    int min_qual_char = 0;        // --min-qual-char=C: windows with a base whose quality byte is below C are not k-mers
    std::string output, histo;    // --output=FILE: "kmer<TAB>count" lines; --histo=FILE: "count<TAB>k-mers" lines
    uint64_t lower = 1, upper = UINT64_MAX;   // --lower / --upper: the counts --output writes
    uint64_t histo_max = 10000;   // --histo-max=H: counts 1..H, then one line H+1 for everything above
    // read queries after the count: --filter=OUT writes the records of --filter-input (default --input) that pass the
    // rule, --read-stats=FILE one line of k-mer stats per record
    std::string filter, filter_input, read_stats;
    uint64_t filter_lower = 2, filter_upper = UINT64_MAX, filter_min = 0;
    double filter_fraction = 1.0;
    bool filter_invert = false;
    // the median rule: --filter-median-lower / -upper switch --filter to it; --read-medians=FILE writes every record's median
    std::string read_medians;
    uint64_t filter_median_lower = 0, filter_median_upper = UINT64_MAX;
    bool filter_median = false, filter_share = false;   // options of the median rule / of the share rule were given
    // read trimming after the count: --trim=OUT writes the records of --trim-input (default --input) cut to their solid
    // stretch, --trim-spans=FILE one line index<TAB>start<TAB>length per record
    std::string trim, trim_input, trim_spans, trim_mode = "longest";
    // paired reads: two comma-separated files in --filter-input / --trim-input (and as many outputs), or one interleaved
    // file; orphans go to --filter-singles / --trim-singles; --pair-names compares the mates' names
    std::string filter_singles, trim_singles, filter_pairs = "both";
    bool filter_interleaved = false, trim_interleaved = false, pair_names = false;
    uint64_t trim_lower = 2, trim_upper = UINT64_MAX, trim_min_len = 0;
    // k-mer databases: --save=DB after the count and the check, --load=DB[,DB2,...] before the count (summed)
    std::string save;
    std::vector<std::string> load;
    // table set operations: --with=DB[,DB2,...] is the second table (summed as --load sums), --op joins the counted /
    // loaded table with it and the result takes its place for everything after the check; --compare prints the overlap
    std::vector<std::string> with;
    std::string op, op_count = "min";
    uint64_t a_lower = 1, a_upper = UINT64_MAX, b_lower = 1, b_upper = UINT64_MAX;
    bool compare = false;
    // joint spectrum of the two tables: --joint-histo=FILE writes how many k-mers occur a times in A and b times in B,
    // counts 0..H per side and one bin H+1 for everything above (--joint-max-a / --joint-max-b), as lines or as a matrix
    std::string joint_histo, joint_format = "sparse";
    uint64_t joint_max_a = 1000, joint_max_b = 1000;
    bool joint_opts = false;   // --joint-max-a / --joint-max-b / --joint-format were given
    // heterozygous pairs of the table: --het-histo=FILE writes how many pairs of k-mers that differ only in their middle
    // base are counted (minor, major) times, counts 0..H per side and one bin H+1 above (--het-max); --het-pairs=FILE the pairs
    std::string het_histo, het_pairs, het_format = "sparse", het_mode = "unique";
    uint64_t het_max = 1000, het_lower = 1, het_upper = UINT64_MAX;
    bool het_opts = false;     // --het-max / --het-format / --het-lower / --het-upper / --het-mode were given
    // read binning by the two tables: the records of --bin-input (default --input) go to --bin-a / --bin-b /
    // --bin-ambiguous / --bin-none by the table they hit more; --bin-stats=FILE writes the hits of every record
    std::string bin_a, bin_b, bin_ambiguous, bin_none, bin_input, bin_stats;
    uint64_t bin_min_hits = 1;
    uint32_t bin_ratio_milli = 1000;
    bool bin_opts = false;     // --bin-min-hits / --bin-ratio were given
    bool given_k = false, given_l = false, given_s = false, given_seed = false;
    // table sizing: --l=auto sketches --input first and counts into the l that holds its k-mers at --load-factor=F;
    // --estimate prints that line and stops
    bool l_auto = false, estimate = false;
    double load_factor = 0.75;
    // --min-count=2: two passes over --input, the first into a prefilter of 2^prefilter_bits bits (0: l + 6), so that k-mers
    // seen once take no slot
    int min_count = 1, prefilter_bits = 0;
    // digital normalization: --normalize=OUT counts --input through tsx_hip_normalize_host instead of the plain count and
    // writes the kept records to OUT
    std::string normalize;
    uint64_t normalize_cutoff = 20, normalize_round = TSX_HIP_NORMALIZE_ROUND;
    bool normalize_opts = false;   // --normalize-cutoff / --normalize-round were given
};

static bool opt(const char *arg, const char *name, std::string &val) {
    std::string a(arg), n = std::string("--") + name;
    if (a == n) { val = ""; return true; }
    if (a.compare(0, n.size() + 1, n + "=") == 0) { val = a.substr(n.size() + 1); return true; }
    return false;
}

static int usage() {
    std::cerr << "Usage: tsxCount [--input=FASTQ|FASTA[.gz]] [--k=K] [--l=L|auto [--load-factor=F]] [--estimate] [--s=STORAGE]\n"
                 "                [--min-count=1|2 [--prefilter-bits=B]]\n"
                 "                [--mode=HIP] [--threads=T]\n"
                 "                [--check] [--checkabort] [--seed=S] [--device=D] [--format=fastq|fasta|fasta-wrapped] [--canonical]\n"
                 "                [--acgt-only] [--min-qual-char=C]\n"
                 "                [--gpus=N [--comm=rccl|copy] [--devices=a,b,...] [--exchange=merge|mini|auto]]\n"
                 "                [--output=FILE [--lower=N] [--upper=N]] [--histo=FILE [--histo-max=H]]\n"
                 "                [--filter=OUT] [--read-stats=FILE] [--filter-input=FILE] [--filter-lower=N] [--filter-upper=N]\n"
                 "                [--filter-min=M] [--filter-fraction=F] [--filter-invert] [--save=DB] [--load=DB[,DB2,...]]\n"
                 "                [--read-medians=FILE] [--filter-median-lower=N] [--filter-median-upper=N]\n"
                 "                [--normalize=OUT [--normalize-cutoff=20] [--normalize-round=65536]]\n"
                 "                [--trim=OUT] [--trim-spans=FILE] [--trim-input=FILE] [--trim-lower=N] [--trim-upper=N]\n"
                 "                [--trim-mode=longest|prefix] [--trim-min-len=N]\n"
                 "                [--filter-input=R1,R2 --filter=O1,O2] [--filter-singles=S1,S2] [--filter-pairs=both|any]\n"
                 "                [--filter-interleaved] [--trim-input=R1,R2 --trim=O1,O2] [--trim-singles=S1,S2]\n"
                 "                [--trim-interleaved] [--pair-names]\n"
                 "                [--with=DB[,DB2,...] [--op=intersect|union|subtract|diff] [--op-count=min|max|sum|left|right]\n"
                 "                 [--a-lower=N] [--a-upper=N] [--b-lower=N] [--b-upper=N] [--compare]\n"
                 "                 [--joint-histo=FILE [--joint-max-a=H] [--joint-max-b=H] [--joint-format=sparse|matrix]]\n"
                 "                 [--bin-a=OUT] [--bin-b=OUT] [--bin-ambiguous=OUT] [--bin-none=OUT] [--bin-input=FILE]\n"
                 "                 [--bin-stats=FILE] [--bin-min-hits=N] [--bin-ratio=R]]\n"
                 "                [--het-histo=FILE [--het-max=H] [--het-format=sparse|matrix]] [--het-pairs=FILE]\n"
                 "                [--het-lower=N] [--het-upper=N] [--het-mode=unique|all]\n"
                 "Count k-mers on an MI355X. --check compares with FASTQ.<k>.count (kmer<TAB>count per line).\n"
                 "--l=auto sizes the table itself: the input is sketched first (HyperLogLog, 2^14 registers, on the GPU), and l\n"
                 "is the smallest table that holds the estimated distinct k-mers at load F (--load-factor, default 0.75, at most\n"
                 "0.9) with a margin of five standard errors; it prints estimate<TAB>kmers<TAB>distinct<TAB>l<TAB>load, then counts.\n"
                 "--estimate prints that line and stops: nothing is counted, --k is required, --l is ignored. Both take plain,\n"
                 ".gz and BGZF input with --canonical, --acgt-only and --min-qual-char; one GPU, no --load / --with, no wrapped\n"
                 "FASTA. l is at most min(36, 2k - 1): where that leaves the load above 0.9 a warning says so.\n"
                 "--min-count=2 keeps the k-mers that occur once out of the table: the input is read twice, first into a Bloom\n"
                 "prefilter of 2^B bits (--prefilter-bits=B, 12 .. 38, default l + 6) and a second one a quarter its size, then\n"
                 "counted; only k-mers the filter has seen twice are inserted. Every k-mer that occurs twice or more has its exact\n"
                 "count; one that occurs once is absent or, seldom, there with count 1: --output --lower=2, --histo from 2 on,\n"
                 "--filter and --trim at their default lower bound are those of a plain count. It prints\n"
                 "prefilter<TAB>bits<TAB>kmers<TAB>seen_again<TAB>admitted<TAB>skipped. One GPU; no --check, --load, --l=auto or\n"
                 "wrapped FASTA. A --save made this way holds no complete set of the k-mers seen once.\n"
                 "--format=fasta reads two lines per record (a header, ONE sequence line), as file names ending in .fa, .fasta\n"
                 "or .fna do. --format=fasta-wrapped reads FASTA whose sequences are wrapped over several lines (what genome and\n"
                 "assembly downloads look like): the lines of a record are joined on the GPU, k-mers across line breaks count.\n"
                 "It names the format of --input only (a --filter-input goes by its own file name), runs on one GPU, and has no\n"
                 "--min-qual-char and no --filter / --read-stats of the wrapped input itself.\n"
                 "--canonical counts a k-mer and its reverse complement as one (the check then expects f(x) + f(rc x)).\n"
                 "--acgt-only skips every k-mer with a byte outside ACGTacgt (an N, say); --min-qual-char=C every k-mer with a\n"
                 "base whose quality byte is below the character C, or that has none (FASTQ only). Both hold for the read\n"
                 "queries too.\n"
                 "--output writes every k-mer counted lower..upper times (default 1..unbounded) as kmer<TAB>count, in no\n"
                 "particular order. --histo writes count<TAB>number of k-mers for every count 1..H (default 10000) that\n"
                 "occurs, then H+1<TAB>number of k-mers counted more than H times.\n"
                 "After the count, --filter writes the records of --filter-input (default: --input) whose k-mers pass: a\n"
                 "k-mer is in range when its count lies in filter-lower..filter-upper (default 2..unbounded); a record passes\n"
                 "with at least M (default 0) k-mers in range that make at least the share F (default 1.0) of its k-mers.\n"
                 "--filter-invert writes the records that fail. --read-stats writes index<TAB>kmers<TAB>in_range<TAB>min<TAB>sum\n"
                 "per record of the same input. One GPU only.\n"
                 "--read-medians writes index<TAB>kmers<TAB>median per record of that input: the median count of the record's\n"
                 "k-mers (the upper middle for an even number, 0 without k-mers). --filter-median-lower=N and / or\n"
                 "--filter-median-upper=N switch --filter to the median rule: a record passes when its median lies in N..N\n"
                 "(default 0..unbounded); --filter-invert applies, the other --filter-* rule options do not go with it. One GPU,\n"
                 "single-end input, no wrapped FASTA.\n"
                 "--normalize=OUT counts --input by digital normalization (khmer's normalize-by-median) instead of the plain\n"
                 "count: the records are taken in rounds of --normalize-round (default 65536) records; a record is kept when the\n"
                 "median count of its k-mers, among the records kept in the rounds before, is below --normalize-cutoff (default\n"
                 "20), and only the k-mers of kept records are counted. The kept records go to OUT, whole and in input order; it\n"
                 "prints normalize<TAB>records<TAB>kept<TAB>kmers_seen<TAB>kmers_added<TAB>rounds. --normalize-round=1 is khmer's\n"
                 "sequential rule; the result depends on the round size. --output, --histo, --save, --filter, --trim,\n"
                 "--read-medians and --with then see the table of the kept reads; --load first normalizes on top of a saved\n"
                 "table. Plain, .gz and BGZF input; --canonical, --acgt-only and --min-qual-char apply. One GPU, single-end; no\n"
                 "--check, --min-count=2, --l=auto / --estimate or wrapped FASTA.\n"
                 "--trim writes the records of --trim-input (default: --input) cut to their solid stretch: a window is solid\n"
                 "when its count lies in trim-lower..trim-upper (default 2..unbounded); --trim-mode=longest keeps the longest run\n"
                 "of solid windows (the leftmost among equals), prefix the run that starts the read. Records that keep fewer\n"
                 "than trim-min-len bases (default k) are dropped. --trim-spans writes index<TAB>start<TAB>length per record.\n"
                 "Paired reads stay in step: --filter-input=R1,R2 --filter=O1,O2 (or --filter-interleaved with one file each)\n"
                 "takes record i of R1 and record i of R2 as one pair (interleaved: records 2i and 2i+1). --filter-pairs=both\n"
                 "(default) keeps a pair when both mates pass, any when one does; under both a mate that passes alone goes to\n"
                 "--filter-singles=S1,S2 (interleaved: S), or is dropped. --trim-input=R1,R2 --trim=O1,O2 [--trim-singles=S1,S2]\n"
                 "and --trim-interleaved do the same for the trim: a pair is kept when both mates are written, a lone survivor is\n"
                 "an orphan. --pair-names compares the mates' names (the header up to the first blank, without a trailing /1 or\n"
                 "/2). Different record counts, an odd interleaved file or differing names stop the run. Prints\n"
                 "pairs<TAB>seen<TAB>kept<TAB>single1<TAB>single2 (the trim adds <TAB>bases_in<TAB>bases_kept). Each file goes by its\n"
                 "own name (plain, .gz, BGZF); no --read-stats / --trim-spans, no wrapped FASTA, one GPU.\n"
                 "Prints trim<TAB>records<TAB>kept<TAB>bases_in<TAB>bases_kept. One GPU only; --trim-input goes by its own file\n"
                 "name and is never wrapped FASTA.\n"
                 "--save writes the table as a k-mer database after the count and the check. --load fills the table from\n"
                 "k-mer databases first (several are summed); the first sets k, l, s and the seed unless they are given, a\n"
                 "different l or s re-inserts every k-mer. --input is then optional: its reads are counted on top of the\n"
                 "loaded counts. --load refuses --check; --filter and --read-stats without --input need --filter-input.\n"
                 "--canonical, --acgt-only and --min-qual-char must match the databases. One GPU only.\n"
                 "--with names a second table B (databases, summed); A is the table as --load and --input leave it. --op joins\n"
                 "them after the count and the check: intersect (k-mers of both), union (of either), subtract (A's k-mers that\n"
                 "B lacks, with A's count), diff (count differences a - b > 0). --op-count picks the count of a k-mer that is\n"
                 "in both: min (default), max, sum, left (A's), right (B's). --a-lower/--a-upper and --b-lower/--b-upper keep\n"
                 "only the k-mers of A / B counted that often. The result takes the table's place for --output, --histo,\n"
                 "--save, --filter and --read-stats. --compare prints compare<TAB>a<TAB>b<TAB>both<TAB>jaccard (distinct k-mers\n"
                 "of A, of B, of both, Jaccard index) and the summed counts of the shared k-mers. B must match A's k,\n"
                 "--canonical, --acgt-only and --min-qual-char. One GPU only.\n"
                 "--joint-histo=FILE writes the joint spectrum of A and B (before --op replaces the table): how many distinct\n"
                 "k-mers occur a times in A and b times in B, 0 for a table that lacks the k-mer. --joint-max-a=H and\n"
                 "--joint-max-b=H (default 1000) give counts 0..H and one bin H+1 for everything above, per side.\n"
                 "--joint-format=sparse (default) writes a<TAB>b<TAB>k-mers for every pair that occurs, ordered by a, then b;\n"
                 "matrix writes a comment line, then H+2 lines of H+2 numbers, the line being the count in A. It prints\n"
                 "joint<TAB>a_only<TAB>b_only<TAB>both (distinct k-mers). It needs --with; one GPU only.\n"
                 "--bin-a=OUT and --bin-b=OUT split the records of --bin-input (default: --input; plain, .gz or BGZF) by the\n"
                 "table they belong to, in one scan against A and B (before --op replaces the table): a k-mer of a read hits A\n"
                 "when its count there lies in --a-lower..--a-upper, B with --b-lower..--b-upper. A read goes to the table it\n"
                 "hits more, given at least --bin-min-hits=N hits (default 1) and at least R times the other table's hits\n"
                 "(--bin-ratio=R, a decimal 1 .. 1000, default 1, three places kept); ties and reads no side wins go to\n"
                 "--bin-ambiguous=OUT, reads that reach N hits in neither table to --bin-none=OUT. An output that is not named\n"
                 "is counted and not written. --bin-stats=FILE writes\n"
                 "index<TAB>kmers<TAB>hits_a<TAB>hits_b<TAB>hits_both<TAB>class per record (class: a, b, ambiguous, none). It\n"
                 "prints bin<TAB>records<TAB>a<TAB>b<TAB>ambiguous<TAB>none. It needs --with; single-end input, no wrapped\n"
                 "FASTA, one GPU only.\n"
                 "--het-histo=FILE writes the heterozygous k-mer pairs of the table (Smudgeplot's hetkmers): how many pairs of\n"
                 "k-mers that differ only in their middle base are counted `minor` and `major` times (minor <= major), over the\n"
                 "k-mers counted --het-lower=N (default 1) to --het-upper=N times. --het-mode=unique (default) counts a pair only\n"
                 "when no third k-mer shares its flanks, all counts every pair. --het-max=H (default 1000, at most 4094) gives\n"
                 "counts 0..H and one bin H+1 above, per side; --het-format=sparse (default) writes minor<TAB>major<TAB>pairs for\n"
                 "every cell that occurs, ordered by minor, then major; matrix writes a comment line, then H+2 lines of H+2\n"
                 "numbers, the line being the minor count. --het-pairs=FILE writes the pairs themselves as\n"
                 "minor_kmer<TAB>minor_count<TAB>major_kmer<TAB>major_count. Either prints\n"
                 "het<TAB>kmers<TAB>paired<TAB>pairs<TAB>families2<TAB>families3plus. They run where --histo runs, on the table\n"
                 "as --load / --input leave it and before --op replaces it. k must be odd; one GPU only."
              << std::endl;
    return 1;
}

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

// whole input in memory: plain files are mmap'ed; .gz (FastXReader.h:178-206 picks zlib mode by the same suffix
// test): a blocked gzip file (BGZF) is mmap'ed as it is and inflated on the GPU (bgzf = true), any other gzip
// stream goes through zlib here
static bool load_input(const std::string &path, std::vector<char> &owned, const char *&text, size_t &n, void *&map,
                       bool &bgzf, bool allow_bgzf) {
    map = nullptr;
    bgzf = false;
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
                    map = zm; text = (const char *)zm; n = (size_t)zst.st_size; bgzf = true;
                    return true;
                }
                munmap(zm, (size_t)zst.st_size);
            }
        }
        if (zfd >= 0) close(zfd);
        const bool ok = read_gz(path, owned);
        text = owned.data(); n = owned.size();
        return ok;
    }
    int fd = open(path.c_str(), O_RDONLY);
    if (fd < 0) return false;
    struct stat st;
    if (fstat(fd, &st) != 0) { close(fd); return false; }
    n = (size_t)st.st_size;
    if (n == 0) { close(fd); text = ""; return true; }
    map = mmap(nullptr, n, PROT_READ, MAP_PRIVATE, fd, 0);
    close(fd);
    if (map == MAP_FAILED) { map = nullptr; return false; }
    text = (const char *)map;
    return true;
}

static bool is_wrapped(const arguments &a) { return a.format == "fasta-wrapped"; }   // multi-line FASTA, lines joined on the GPU

static bool is_fasta(const arguments &a) {   // FASTA (two lines per record, FASTXreader<FASTAEntry>) by option or by file name
    std::string stem = a.input_path;
    if (stem.size() > 3 && stem.rfind(".gz") == stem.size() - 3) stem.resize(stem.size() - 3);
    auto ends = [&](const char *suf) { const std::string x(suf); return stem.size() >= x.size() && stem.compare(stem.size() - x.size(), x.size(), x) == 0; };
    return a.format == "fasta" || (a.format.empty() && (ends(".fa") || ends(".fasta") || ends(".fna")));
}

// reverse complement of an ACGT string (what --canonical --check pairs up)
static std::string revcomp(const std::string &s) {
    std::string r(s.rbegin(), s.rend());
    for (char &c : r) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : c;
    return r;
}

// --het-histo and --het-pairs: the heterozygous pairs of the table as files, and their totals on stdout
static void write_het(TSXHashMapHIP &oMap, const arguments &a) {
    if (a.het_histo.empty() && a.het_pairs.empty()) return;
    const tsx_hip_het_rule oRule = {a.het_lower, a.het_upper, a.het_mode == "all" ? TSX_HIP_HET_ALL : TSX_HIP_HET_UNIQUE, 0};
    const size_t nb = (size_t)a.het_max + 2;
    std::vector<uint64_t> m;
    const tsx_hip_het_stats s = oMap.hetHistogram(oRule, nb, nb, m);
    if (!a.het_histo.empty()) {
        std::ofstream f(a.het_histo);
        if (a.het_format == "matrix") f << "# rows: minor count 0.." << nb - 1 << ", columns: major count\n";
        for (size_t i = 0; i < nb; ++i) {
            for (size_t j = 0; j < nb; ++j) {
                const uint64_t n = m[i * nb + j];
                if (a.het_format == "matrix") f << n << (j + 1 < nb ? '\t' : '\n');
                else if (n) f << i << '\t' << j << '\t' << n << '\n';
            }
        }
        f.close();
        if (!f) throw TSXException("could not write " + a.het_histo, TSX_HIP_EIO);
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
    if (!a.het_histo.empty() || !a.het_pairs.empty())
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
        std::ofstream f(a.histo);
        for (uint64_t c = 1; c <= a.histo_max; ++c)
            if (h[c]) f << c << '\t' << h[c] << '\n';
        f << a.histo_max + 1 << '\t' << h[a.histo_max + 1] << '\n';
        f.close();
        if (!f) throw TSXException("could not write " + a.histo, TSX_HIP_EIO);
        std::cerr << "Wrote the count histogram to " << a.histo << std::endl;
    }
}

static bool is_fasta_path(const std::string &path, const std::string &format) {
    arguments b;
    b.input_path = path;
    b.format = format;
    return is_fasta(b);
}

static std::vector<std::string> split_commas(const std::string &s) {
    std::vector<std::string> out;
    size_t at = 0;
    for (;;) {
        const size_t c = s.find(',', at);
        out.push_back(s.substr(at, c == std::string::npos ? c : c - at));
        if (c == std::string::npos) return out;
        at = c + 1;
    }
}
static bool filter_paired(const arguments &a) { return a.filter_interleaved || a.filter_input.find(',') != std::string::npos; }
static bool trim_paired(const arguments &a) { return a.trim_interleaved || a.trim_input.find(',') != std::string::npos; }

// One text of a paired run, loaded as the filter's input is (a BGZF file is inflated on the device).
struct pair_text {
    std::vector<char> owned;
    const char *text = nullptr;
    size_t n = 0;
    void *map = nullptr;
    ~pair_text() { if (map) munmap(map, n); }
    template <typename C>
    bool load(const std::string &path, int device, C check) {
        bool bgzf = false;
        if (!load_input(path, owned, text, n, map, bgzf, true)) {
            std::cerr << "Could not read " << path << std::endl;
            return false;
        }
        if (bgzf) {
            size_t members = 0, tb = 0, got = 0;
            check(tsx_hip_bgzf_index_host(text, n, &members, &tb));
            std::vector<char> inflated(tb ? tb : 1);
            check(tsx_hip_inflate_bgzf_host(device, text, n, inflated.data(), tb, &got));
            munmap(map, n);
            map = nullptr;
            owned.swap(inflated);
            owned.resize(got);
            text = owned.data();
            n = got;
        }
        return true;
    }
};

// --filter / --trim over mate pairs: two files or one interleaved file, where the single-end forms run.
static int run_pairs(tsx_hip_map *pMap, const arguments &a, bool trim) {
    auto check = [](int rc) {
        if (rc == TSX_HIP_OK) return;
        std::string msg = tsx_hip_strerror(rc);
        if (rc == TSX_HIP_EHIP || rc == TSX_HIP_EIO || rc == TSX_HIP_ENOMEM || rc == TSX_HIP_EPAIR)
            msg += std::string(" (") + tsx_hip_last_error() + ")";
        throw TSXException(msg, rc);
    };
    const std::vector<std::string> in = split_commas(trim ? a.trim_input : a.filter_input);
    const std::vector<std::string> out = split_commas(trim ? a.trim : a.filter);
    const std::string &singles = trim ? a.trim_singles : a.filter_singles;
    const std::vector<std::string> sg = singles.empty() ? std::vector<std::string>() : split_commas(singles);
    const bool inter = in.size() == 1;
    pair_text t1, t2;
    if (!t1.load(in[0], a.device, check) || (!inter && !t2.load(in[1], a.device, check))) return 3;
    const bool fa = is_fasta_path(in[0], is_wrapped(a) ? std::string() : a.format);
    if (!inter && fa != is_fasta_path(in[1], is_wrapped(a) ? std::string() : a.format)) {
        std::cerr << "paired input: " << in[0] << " and " << in[1] << " differ in format" << std::endl;
        return 3;
    }
    check(tsx_hip_set_record_lines(pMap, fa ? 2 : 4));
    const std::string paths[4] = {out[0], inter ? std::string() : out[1], sg.empty() ? std::string() : sg[0],
                                  sg.size() > 1 ? sg[1] : std::string()};
    tsx_hip_pair_totals t;
    if (trim) {
        tsx_hip_trim_rule rule;
        rule.lower = a.trim_lower;
        rule.upper = a.trim_upper;
        rule.min_len = a.trim_min_len;
        rule.mode = a.trim_mode == "prefix" ? TSX_HIP_TRIM_PREFIX : TSX_HIP_TRIM_LONGEST;
        rule.reserved = 0;
        t = tsx_trim_pairs(pMap, t1.text, t1.n, inter ? nullptr : t2.text, t2.n, rule, a.pair_names, paths, 0, check);
        std::cout << "pairs\t" << t.pairs << '\t' << t.kept << '\t' << t.single1 << '\t' << t.single2 << '\t' << t.bases_in << '\t'
                  << t.bases_kept << std::endl;
    } else {
        tsx_hip_filter_rule rule;
        rule.lower = a.filter_lower;
        rule.upper = a.filter_upper;
        rule.min_in_range = a.filter_min;
        rule.fraction_ppm = (uint32_t)std::llround(a.filter_fraction * 1e6);
        rule.invert = a.filter_invert ? 1 : 0;
        t = tsx_filter_pairs(pMap, t1.text, t1.n, inter ? nullptr : t2.text, t2.n, rule,
                             a.filter_pairs == "any" ? TSX_HIP_PAIR_ANY : TSX_HIP_PAIR_BOTH, a.pair_names, paths, 0, check);
        std::cout << "pairs\t" << t.pairs << '\t' << t.kept << '\t' << t.single1 << '\t' << t.single2 << std::endl;
    }
    std::cerr << "Wrote " << t.kept << " of " << t.pairs << " pairs (" << t.bytes1 + t.bytes2 << " bytes), " << t.single1 << " + "
              << t.single2 << " single mates" << std::endl;
    return 0;
}

// What the paired forms of --filter (trim = false) and --trim refuse; an empty string when all is well.
static std::string pairs_refusal(const arguments &a, bool trim) {
    const std::string opt = trim ? "--trim" : "--filter";
    const std::string &in = trim ? a.trim_input : a.filter_input, &out = trim ? a.trim : a.filter;
    const std::string &singles = trim ? a.trim_singles : a.filter_singles;
    const bool inter = trim ? a.trim_interleaved : a.filter_interleaved;
    const size_t want = inter ? 1 : 2;
    if (!(trim ? a.trim_spans : a.read_stats).empty())
        return (trim ? std::string("--trim-spans") : std::string("--read-stats")) + " does not go with paired input";
    if (in.empty()) return opt + "-interleaved needs " + opt + "-input=FILE";
    if (out.empty()) return "paired input needs " + opt + "=" + (inter ? "OUT" : "O1,O2");
    if (split_commas(in).size() != want || split_commas(out).size() != want || (!singles.empty() && split_commas(singles).size() != want))
        return opt + "-input, " + opt + " and " + opt + "-singles must name " + (inter ? "one file each with " + opt + "-interleaved"
                                                                                  : "two files each (R1,R2)");
    for (const std::string &p : split_commas(in + "," + out + (singles.empty() ? "" : "," + singles)))
        if (p.empty()) return "an empty file name in the paired " + opt + " options";
    if (a.gpus > 1) return "paired " + opt + " runs on one GPU only";
    return "";
}

static bool wants_queries(const arguments &a) { return !a.filter.empty() || !a.read_stats.empty() || !a.read_medians.empty(); }
static bool wants_medians(const arguments &a) { return !a.read_medians.empty() || a.filter_median; }

// --filter and --read-stats on one table, after the count, the check and --output / --histo.  The input loads as the
// counted one does; a BGZF file is inflated on the device.
static int run_read_queries(tsx_hip_map *pMap, const arguments &a) {
    auto check = [](int rc) {
        if (rc == TSX_HIP_OK) return;
        std::string msg = tsx_hip_strerror(rc);
        if (rc == TSX_HIP_EHIP || rc == TSX_HIP_EIO || rc == TSX_HIP_ENOMEM) msg += std::string(" (") + tsx_hip_last_error() + ")";
        throw TSXException(msg, rc);
    };
    const std::string path = a.filter_input.empty() ? a.input_path : a.filter_input;
    std::vector<char> owned;
    const char *text = nullptr;
    size_t n = 0;
    void *map = nullptr;
    bool bgzf = false;
    if (!load_input(path, owned, text, n, map, bgzf, true)) {
        std::cerr << "Could not read " << path << std::endl;
        return 3;
    }
    if (bgzf) {
        size_t members = 0, tb = 0, got = 0;
        check(tsx_hip_bgzf_index_host(text, n, &members, &tb));
        std::vector<char> inflated(tb ? tb : 1);
        check(tsx_hip_inflate_bgzf_host(a.device, text, n, inflated.data(), tb, &got));
        munmap(map, n);
        map = nullptr;
        owned.swap(inflated);
        owned.resize(got);
        text = owned.data();
        n = got;
    }
    // (--format=fasta-wrapped names the format of --input only: the queried file goes by its name)
    check(tsx_hip_set_record_lines(pMap, is_fasta_path(path, is_wrapped(a) ? std::string() : a.format) ? 2 : 4));
    if (!a.read_stats.empty()) {
        const std::vector<tsx_hip_read_stats> st = tsx_query_reads(pMap, text, n, a.filter_lower, a.filter_upper, 0, check);
        std::ofstream f(a.read_stats);
        for (size_t i = 0; i < st.size(); ++i)
            f << i << '\t' << st[i].kmers << '\t' << st[i].in_range << '\t' << st[i].min_count << '\t' << st[i].sum_count << '\n';
        f.close();
        if (!f) throw TSXException("could not write " + a.read_stats, TSX_HIP_EIO);
        std::cerr << "Wrote the k-mer stats of " << st.size() << " records to " << a.read_stats << std::endl;
    }
    if (!a.read_medians.empty()) {
        const std::vector<tsx_hip_read_median> md = tsx_median_reads(pMap, text, n, 0, check);
        std::ofstream f(a.read_medians);
        for (size_t i = 0; i < md.size(); ++i) f << i << '\t' << md[i].kmers << '\t' << md[i].median << '\n';
        f.close();
        if (!f) throw TSXException("could not write " + a.read_medians, TSX_HIP_EIO);
        std::cerr << "Wrote the median k-mer counts of " << md.size() << " records to " << a.read_medians << std::endl;
    }
    if (!a.filter.empty() && a.filter_median) {
        tsx_hip_median_rule rule;
        rule.lower = a.filter_median_lower;
        rule.upper = a.filter_median_upper;
        rule.invert = a.filter_invert ? 1 : 0;
        rule.reserved = 0;
        const std::pair<uint64_t, uint64_t> r = tsx_filter_median(pMap, text, n, rule, a.filter, 0, check);
        std::cerr << "Wrote " << r.first << " records (" << r.second << " bytes) to " << a.filter << std::endl;
    } else if (!a.filter.empty()) {
        tsx_hip_filter_rule rule;
        rule.lower = a.filter_lower;
        rule.upper = a.filter_upper;
        rule.min_in_range = a.filter_min;
        rule.fraction_ppm = (uint32_t)std::llround(a.filter_fraction * 1e6);
        rule.invert = a.filter_invert ? 1 : 0;
        const std::pair<uint64_t, uint64_t> r = tsx_filter_reads(pMap, text, n, rule, a.filter, 0, check);
        std::cerr << "Wrote " << r.first << " records (" << r.second << " bytes) to " << a.filter << std::endl;
    }
    if (map) munmap(map, n);
    return 0;
}

static bool wants_trim(const arguments &a) { return !a.trim.empty() || !a.trim_spans.empty(); }

// --trim and --trim-spans on one table, where --filter runs.  The input loads as the filter's does.
static int run_trim(tsx_hip_map *pMap, const arguments &a) {
    auto check = [](int rc) {
        if (rc == TSX_HIP_OK) return;
        std::string msg = tsx_hip_strerror(rc);
        if (rc == TSX_HIP_EHIP || rc == TSX_HIP_EIO || rc == TSX_HIP_ENOMEM) msg += std::string(" (") + tsx_hip_last_error() + ")";
        throw TSXException(msg, rc);
    };
    const std::string path = a.trim_input.empty() ? a.input_path : a.trim_input;
    std::vector<char> owned;
    const char *text = nullptr;
    size_t n = 0;
    void *map = nullptr;
    bool bgzf = false;
    if (!load_input(path, owned, text, n, map, bgzf, true)) {
        std::cerr << "Could not read " << path << std::endl;
        return 3;
    }
    if (bgzf) {
        size_t members = 0, tb = 0, got = 0;
        check(tsx_hip_bgzf_index_host(text, n, &members, &tb));
        std::vector<char> inflated(tb ? tb : 1);
        check(tsx_hip_inflate_bgzf_host(a.device, text, n, inflated.data(), tb, &got));
        munmap(map, n);
        map = nullptr;
        owned.swap(inflated);
        owned.resize(got);
        text = owned.data();
        n = got;
    }
    check(tsx_hip_set_record_lines(pMap, is_fasta_path(path, is_wrapped(a) ? std::string() : a.format) ? 2 : 4));
    tsx_hip_trim_rule rule;
    rule.lower = a.trim_lower;
    rule.upper = a.trim_upper;
    rule.min_len = a.trim_min_len;
    rule.mode = a.trim_mode == "prefix" ? TSX_HIP_TRIM_PREFIX : TSX_HIP_TRIM_LONGEST;
    rule.reserved = 0;
    if (!a.trim_spans.empty()) {
        const std::vector<tsx_hip_trim_span> sp = tsx_trim_spans(pMap, text, n, rule, 0, check);
        std::ofstream f(a.trim_spans);
        for (size_t i = 0; i < sp.size(); ++i) f << i << '\t' << sp[i].start << '\t' << sp[i].length << '\n';
        f.close();
        if (!f) throw TSXException("could not write " + a.trim_spans, TSX_HIP_EIO);
        std::cerr << "Wrote the kept spans of " << sp.size() << " records to " << a.trim_spans << std::endl;
    }
    if (!a.trim.empty()) {
        const tsx_hip_trim_totals t = tsx_trim_reads(pMap, text, n, rule, a.trim, 0, check);
        std::cout << "trim\t" << t.records << '\t' << t.kept << '\t' << t.bases_in << '\t' << t.bases_kept << std::endl;
        std::cerr << "Wrote " << t.kept << " trimmed records (" << t.bytes << " bytes) to " << a.trim << std::endl;
    }
    if (map) munmap(map, n);
    return 0;
}

// what follows the count, the check, the outputs and the set operation: the read queries, then the trim
static int run_after(tsx_hip_map *pMap, const arguments &a) {
    const int rq = !wants_queries(a) ? 0 : filter_paired(a) ? run_pairs(pMap, a, false) : run_read_queries(pMap, a);
    const int rt = !wants_trim(a) ? 0 : trim_paired(a) ? run_pairs(pMap, a, true) : run_trim(pMap, a);
    return rq ? rq : rt;
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
    std::ofstream f(a.joint_histo);
    if (a.joint_format == "matrix")
        f << "# rows: count in A 0.." << na - 1 << ", columns: count in B\n";
    for (size_t i = 0; i < na; ++i) {
        for (size_t j = 0; j < nb; ++j) {
            const uint64_t n = m[i * nb + j];
            (i == 0 ? b_only : j == 0 ? a_only : both) += n;
            if (a.joint_format == "matrix") f << n << (j + 1 < nb ? '\t' : '\n');
            else if (n) f << i << '\t' << j << '\t' << n << '\n';
        }
    }
    f.close();
    if (!f) throw TSXException("could not write " + a.joint_histo, TSX_HIP_EIO);
    std::cout << "joint\t" << a_only << '\t' << b_only << '\t' << both << std::endl;
    std::cerr << "Wrote the joint histogram to " << a.joint_histo << std::endl;
}

// --bin-ratio: digits[.digits], 1 .. 1000, in thousandths (the decimals behind the third are dropped)
static bool parse_ratio_milli(const std::string &v, uint32_t &milli) {
    size_t i = 0;
    uint64_t whole = 0, frac = 0;
    int places = 0;
    for (; i < v.size() && v[i] >= '0' && v[i] <= '9'; ++i) whole = std::min<uint64_t>(whole * 10 + (uint64_t)(v[i] - '0'), 1000000);
    if (i == 0) return false;
    if (i < v.size() && v[i] == '.') {
        const size_t dot = i++;
        for (; i < v.size() && v[i] >= '0' && v[i] <= '9'; ++i)
            if (places < 3) { frac = frac * 10 + (uint64_t)(v[i] - '0'); ++places; }
        if (i == dot + 1) return false;
    }
    if (i != v.size()) return false;
    for (; places < 3; ++places) frac *= 10;
    const uint64_t m = whole * 1000 + frac;
    if (m < 1000 || m > 1000000) return false;
    milli = (uint32_t)m;
    return true;
}

static bool wants_bin(const arguments &a) {
    return !a.bin_a.empty() || !a.bin_b.empty() || !a.bin_ambiguous.empty() || !a.bin_none.empty() || !a.bin_stats.empty();
}
static bool wants_bin_reads(const arguments &a) {
    return !a.bin_a.empty() || !a.bin_b.empty() || !a.bin_ambiguous.empty() || !a.bin_none.empty();
}

// --bin-*: the records of --bin-input by the table they hit more, where --compare and --joint-histo run
static int run_bin(TSXHashMapHIP &oA, TSXHashMapHIP &oB, const arguments &a) {
    auto check = [](int rc) {
        if (rc == TSX_HIP_OK) return;
        throw TSXException(std::string(tsx_hip_strerror(rc)) + " (" + tsx_hip_last_error() + ")", rc);
    };
    const std::string path = a.bin_input.empty() ? a.input_path : a.bin_input;
    pair_text t;   // (loaded as every read query's input: a BGZF file is inflated on the device)
    if (!t.load(path, a.device, check)) return 3;
    oA.setRecordLines(is_fasta_path(path, is_wrapped(a) ? std::string() : a.format) ? 2 : 4);
    const tsx_hip_bin_rule rule = {a.a_lower, a.a_upper, a.b_lower, a.b_upper, a.bin_min_hits, a.bin_ratio_milli, 0};
    static const char *const names[4] = {"a", "b", "ambiguous", "none"};
    uint64_t records = 0, n[4] = {0, 0, 0, 0};
    if (!a.bin_stats.empty()) {
        std::vector<uint8_t> cls;
        const std::vector<tsx_hip_bin_stats> st = oA.binStats(oB, t.text, t.n, rule, &cls);
        std::ofstream f(a.bin_stats);
        for (size_t i = 0; i < st.size(); ++i) {
            f << i << '\t' << st[i].kmers << '\t' << st[i].hits_a << '\t' << st[i].hits_b << '\t' << st[i].hits_both << '\t'
              << names[cls[i] & 3] << '\n';
            ++n[cls[i] & 3];
        }
        f.close();
        if (!f) throw TSXException("could not write " + a.bin_stats, TSX_HIP_EIO);
        records = st.size();
        std::cerr << "Wrote the bin stats of " << st.size() << " records to " << a.bin_stats << std::endl;
    }
    if (wants_bin_reads(a)) {
        const std::string paths[4] = {a.bin_a, a.bin_b, a.bin_ambiguous, a.bin_none};
        const tsx_hip_bin_totals bt = oA.binReads(oB, t.text, t.n, rule, paths);
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

// --op / --op-count by name: the TSX_HIP_OP_* / TSX_HIP_CNT_* value, -1 for none given, -2 / -1 for an unknown one
static int op_index(const std::string &s) {
    return s.empty() ? -1 : s == "intersect" ? TSX_HIP_OP_INTERSECT : s == "union" ? TSX_HIP_OP_UNION
         : s == "subtract" ? TSX_HIP_OP_SUBTRACT : s == "diff" ? TSX_HIP_OP_DIFF : -2;
}
static int count_index(const std::string &s) {
    return s == "min" ? TSX_HIP_CNT_MIN : s == "max" ? TSX_HIP_CNT_MAX : s == "sum" ? TSX_HIP_CNT_SUM
         : s == "left" ? TSX_HIP_CNT_LEFT : s == "right" ? TSX_HIP_CNT_RIGHT : -1;
}

// --l=auto and --estimate: the input is sketched on a minimal probe map that carries its counting mode, the estimate of
// its distinct k-mers picks l (a.l, for the count that follows), and one line says so:
// estimate<TAB>kmers<TAB>distinct<TAB>l<TAB>load.
static void size_input(arguments &a, const char *text, size_t n, bool bgzf) {
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
    if (is_fasta(a)) pProbe->setRecordLines(2);
    if (a.canonical) pProbe->setCanonical(true);
    if (a.acgt_only || a.min_qual_char) pProbe->setBaseRule(a.acgt_only, a.min_qual_char);
    t = bgzf ? pProbe->sketchKmersBgzf(text, n, regs) : pProbe->sketchKmers(text, n, regs);
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
    if (is_fasta(a)) { oGroup.setRecordLines(2); std::cerr << "Format=FASTA (2 lines per record)" << std::endl; }
    if (a.canonical) oGroup.setCanonical(true);
    if (a.acgt_only || a.min_qual_char) oGroup.setBaseRule(a.acgt_only, a.min_qual_char);
    // the minimizer exchange where it applies (auto: from 4 GPUs on, as bench.py, and not with --canonical); --exchange=mini
    // insists on it
    const bool rule = a.acgt_only || a.min_qual_char;
    if (a.exchange == "mini" || (a.exchange == "auto" && !a.canonical && !rule && a.gpus >= 4 && a.gpus <= 16 && a.k >= 20 && a.k <= 32)) {
        try { oGroup.setExchange(1); }
        catch (const TSXException &e) { if (a.exchange == "mini") throw; }
    }
    std::cerr << "exchange: " << (oGroup.exchange() == 1 ? "minimizer owners (strip descriptions travel, nothing is merged)" : "per-GPU tables merged") << std::endl;
    std::vector<char> owned;
    const char *text = nullptr;
    size_t n = 0;
    void *map = nullptr;
    bool bgzf = false;
    // (.gz: inflated by zlib on the host, as the reference's reader does -- the record cuts need the text)
    if (!load_input(a.input_path, owned, text, n, map, bgzf, false)) {
        std::cerr << "Could not read " << a.input_path << std::endl;
        return 3;
    }
    auto t0 = std::chrono::steady_clock::now();
    oGroup.countFastq(text, n);
    double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (map) munmap(map, n);
    std::cerr << (oGroup.exchange() == 1 ? "descriptions moved between GPUs by the last share: " : "entries moved between GPUs by the merge: ") << oGroup.exchangedEntries();
    if (oGroup.exchange() == 1) std::cerr << " (exchange rounds: " << oGroup.exchangeRounds() << ")";
    std::cerr << std::endl;
    const int rc = report_and_check(oGroup, a, dt);
    if (!wants_queries(a)) return rc;
    const int rq = run_read_queries(oGroup.rankMap(0), a);   // one GPU: its table holds every k-mer
    return rc ? rc : rq;
}

int main(int argc, char *argv[]) {
    arguments a;
    for (int i = 1; i < argc; ++i) {
        std::string v;
        if (opt(argv[i], "k", v)) { a.k = atoi(v.c_str()); a.given_k = true; }
        else if (opt(argv[i], "l", v)) {
            if (v == "auto") a.l_auto = true;
            else { a.l = atoi(v.c_str()); a.given_l = true; a.l_auto = false; }
        }
        else if (opt(argv[i], "estimate", v)) a.estimate = true;
        else if (opt(argv[i], "load-factor", v)) a.load_factor = atof(v.c_str());
        else if (opt(argv[i], "min-count", v)) {
            if (v != "1" && v != "2") { std::cerr << "--min-count takes 1 (count every k-mer) or 2 (keep k-mers seen once out of the table)" << std::endl; return usage(); }
            a.min_count = atoi(v.c_str());
        }
        else if (opt(argv[i], "prefilter-bits", v)) {
            char *end = nullptr;
            const long b = strtol(v.c_str(), &end, 10);
            if (v.empty() || *end || b < 12 || b > 38) { std::cerr << "--prefilter-bits is the log2 of the prefilter's size in bits: a number 12 .. 38" << std::endl; return usage(); }
            a.prefilter_bits = (int)b;
        }
        else if (opt(argv[i], "s", v)) { a.storagebits = atoi(v.c_str()); a.given_s = true; }
        else if (opt(argv[i], "threads", v)) a.threads = atoi(v.c_str());
        else if (opt(argv[i], "input", v)) a.input_path = v;
        else if (opt(argv[i], "mode", v)) a.mode = v;
        else if (opt(argv[i], "check", v)) a.check = true;
        else if (opt(argv[i], "checkabort", v)) a.checkabort = true;
        else if (opt(argv[i], "seed", v)) { a.seed = strtoull(v.c_str(), nullptr, 10); a.given_seed = true; }
        else if (opt(argv[i], "save", v)) { a.save = v; if (v.empty()) return usage(); }
        else if (opt(argv[i], "load", v) || opt(argv[i], "with", v)) {
            std::vector<std::string> &list = std::string(argv[i]).compare(0, 6, "--load") == 0 ? a.load : a.with;
            for (size_t at = 0; at <= v.size();) {
                const size_t c = v.find(',', at);
                const std::string one = v.substr(at, c == std::string::npos ? std::string::npos : c - at);
                if (one.empty()) return usage();
                list.push_back(one);
                if (c == std::string::npos) break;
                at = c + 1;
            }
        }
        else if (opt(argv[i], "op", v)) { a.op = v; if (v.empty()) return usage(); }
        else if (opt(argv[i], "op-count", v)) a.op_count = v;
        else if (opt(argv[i], "a-lower", v)) a.a_lower = strtoull(v.c_str(), nullptr, 10);
        else if (opt(argv[i], "a-upper", v)) a.a_upper = strtoull(v.c_str(), nullptr, 10);
        else if (opt(argv[i], "b-lower", v)) a.b_lower = strtoull(v.c_str(), nullptr, 10);
        else if (opt(argv[i], "b-upper", v)) a.b_upper = strtoull(v.c_str(), nullptr, 10);
        else if (opt(argv[i], "compare", v)) a.compare = true;
        else if (opt(argv[i], "joint-histo", v)) { a.joint_histo = v; if (v.empty()) return usage(); }
        else if (opt(argv[i], "joint-max-a", v) || opt(argv[i], "joint-max-b", v)) {
            char *end = nullptr;
            errno = 0;
            const unsigned long long h = strtoull(v.c_str(), &end, 10);
            // (H + 2)^2 <= 2^24 for either side: H <= 4094
            if (v.empty() || *end || errno || v[0] == '-' || h < 1 || h > 4094) {
                std::cerr << "--joint-max-a / --joint-max-b take the largest count with a bin of its own: a number 1 .. 4094"
                          << std::endl;
                return usage();
            }
            (std::string(argv[i]).compare(0, 13, "--joint-max-a") == 0 ? a.joint_max_a : a.joint_max_b) = h;
            a.joint_opts = true;
        }
        else if (opt(argv[i], "joint-format", v)) {
            if (v != "sparse" && v != "matrix") { std::cerr << "--joint-format is sparse or matrix" << std::endl; return usage(); }
            a.joint_format = v;
            a.joint_opts = true;
        }
        else if (opt(argv[i], "bin-a", v)) { a.bin_a = v; if (v.empty()) return usage(); }
        else if (opt(argv[i], "bin-b", v)) { a.bin_b = v; if (v.empty()) return usage(); }
        else if (opt(argv[i], "bin-ambiguous", v)) { a.bin_ambiguous = v; if (v.empty()) return usage(); }
        else if (opt(argv[i], "bin-none", v)) { a.bin_none = v; if (v.empty()) return usage(); }
        else if (opt(argv[i], "bin-input", v)) { a.bin_input = v; if (v.empty()) return usage(); }
        else if (opt(argv[i], "bin-stats", v)) { a.bin_stats = v; if (v.empty()) return usage(); }
        else if (opt(argv[i], "bin-min-hits", v)) {
            char *end = nullptr;
            errno = 0;
            a.bin_min_hits = strtoull(v.c_str(), &end, 10);
            if (v.empty() || *end || errno || v[0] == '-') { std::cerr << "--bin-min-hits takes a number" << std::endl; return usage(); }
            a.bin_opts = true;
        }
        else if (opt(argv[i], "bin-ratio", v)) {
            if (!parse_ratio_milli(v, a.bin_ratio_milli)) {
                std::cerr << "--bin-ratio takes a decimal 1 .. 1000 (three places are kept), not '" << v << "'" << std::endl;
                return usage();
            }
            a.bin_opts = true;
        }
        else if (opt(argv[i], "het-histo", v)) { a.het_histo = v; if (v.empty()) return usage(); }
        else if (opt(argv[i], "het-pairs", v)) { a.het_pairs = v; if (v.empty()) return usage(); }
        else if (opt(argv[i], "het-max", v)) {
            char *end = nullptr;
            errno = 0;
            const unsigned long long h = strtoull(v.c_str(), &end, 10);
            // (H + 2)^2 <= 2^24: H <= 4094
            if (v.empty() || *end || errno || v[0] == '-' || h < 1 || h > 4094) {
                std::cerr << "--het-max takes the largest count with a bin of its own: a number 1 .. 4094" << std::endl;
                return usage();
            }
            a.het_max = h;
            a.het_opts = true;
        }
        else if (opt(argv[i], "het-format", v)) {
            if (v != "sparse" && v != "matrix") { std::cerr << "--het-format is sparse or matrix" << std::endl; return usage(); }
            a.het_format = v;
            a.het_opts = true;
        }
        else if (opt(argv[i], "het-mode", v)) {
            if (v != "unique" && v != "all") { std::cerr << "--het-mode is unique or all" << std::endl; return usage(); }
            a.het_mode = v;
            a.het_opts = true;
        }
        else if (opt(argv[i], "het-lower", v) || opt(argv[i], "het-upper", v)) {
            char *end = nullptr;
            errno = 0;
            const unsigned long long c = strtoull(v.c_str(), &end, 10);
            if (v.empty() || *end || errno || v[0] == '-') {
                std::cerr << "--het-lower / --het-upper take a count: a number 0 .. 2^64 - 1" << std::endl;
                return usage();
            }
            (std::string(argv[i]).compare(0, 11, "--het-lower") == 0 ? a.het_lower : a.het_upper) = c;
            a.het_opts = true;
        }
        else if (opt(argv[i], "format", v)) a.format = v;
        else if (opt(argv[i], "device", v)) a.device = atoi(v.c_str());
        else if (opt(argv[i], "gpus", v)) { a.gpus = atoi(v.c_str()); a.group = true; }
        else if (opt(argv[i], "comm", v)) a.comm = v;
        else if (opt(argv[i], "exchange", v)) a.exchange = v;
        else if (opt(argv[i], "canonical", v)) a.canonical = true;
        else if (opt(argv[i], "acgt-only", v)) a.acgt_only = true;
        else if (opt(argv[i], "min-qual-char", v)) {
            if (v.size() != 1) { std::cerr << "--min-qual-char takes one character (e.g. --min-qual-char=5)" << std::endl; return usage(); }
            a.min_qual_char = (unsigned char)v[0];
        }
        else if (opt(argv[i], "output", v)) a.output = v;
        else if (opt(argv[i], "lower", v)) a.lower = strtoull(v.c_str(), nullptr, 10);
        else if (opt(argv[i], "upper", v)) a.upper = strtoull(v.c_str(), nullptr, 10);
        else if (opt(argv[i], "histo", v)) a.histo = v;
        else if (opt(argv[i], "histo-max", v)) a.histo_max = strtoull(v.c_str(), nullptr, 10);
        else if (opt(argv[i], "filter", v)) { a.filter = v; if (v.empty()) return usage(); }
        else if (opt(argv[i], "filter-input", v)) a.filter_input = v;
        else if (opt(argv[i], "filter-lower", v)) { a.filter_lower = strtoull(v.c_str(), nullptr, 10); a.filter_share = true; }
        else if (opt(argv[i], "filter-upper", v)) { a.filter_upper = strtoull(v.c_str(), nullptr, 10); a.filter_share = true; }
        else if (opt(argv[i], "filter-min", v)) { a.filter_min = strtoull(v.c_str(), nullptr, 10); a.filter_share = true; }
        else if (opt(argv[i], "filter-fraction", v)) { a.filter_fraction = atof(v.c_str()); a.filter_share = true; }
        else if (opt(argv[i], "filter-median-lower", v)) { a.filter_median_lower = strtoull(v.c_str(), nullptr, 10); a.filter_median = true; }
        else if (opt(argv[i], "filter-median-upper", v)) { a.filter_median_upper = strtoull(v.c_str(), nullptr, 10); a.filter_median = true; }
        else if (opt(argv[i], "read-medians", v)) { a.read_medians = v; if (v.empty()) return usage(); }
        else if (opt(argv[i], "normalize", v)) { a.normalize = v; if (v.empty()) return usage(); }
        else if (opt(argv[i], "normalize-cutoff", v) || opt(argv[i], "normalize-round", v)) {
            char *end = nullptr;
            const unsigned long long x = strtoull(v.c_str(), &end, 10);
            const bool round = std::string(argv[i]).compare(0, 17, "--normalize-round") == 0;
            if (v.empty() || *end || v[0] == '-' || (round && x == 0)) {
                std::cerr << (round ? "--normalize-round takes a number of records, 1 or more" : "--normalize-cutoff takes a count, 0 or more") << std::endl;
                return usage();
            }
            (round ? a.normalize_round : a.normalize_cutoff) = x;
            a.normalize_opts = true;
        }
        else if (opt(argv[i], "filter-invert", v)) a.filter_invert = true;
        else if (opt(argv[i], "trim", v)) { a.trim = v; if (v.empty()) return usage(); }
        else if (opt(argv[i], "trim-spans", v)) { a.trim_spans = v; if (v.empty()) return usage(); }
        else if (opt(argv[i], "trim-input", v)) a.trim_input = v;
        else if (opt(argv[i], "trim-lower", v)) a.trim_lower = strtoull(v.c_str(), nullptr, 10);
        else if (opt(argv[i], "trim-upper", v)) a.trim_upper = strtoull(v.c_str(), nullptr, 10);
        else if (opt(argv[i], "trim-mode", v)) a.trim_mode = v;
        else if (opt(argv[i], "trim-min-len", v)) a.trim_min_len = strtoull(v.c_str(), nullptr, 10);
        else if (opt(argv[i], "filter-singles", v)) a.filter_singles = v;
        else if (opt(argv[i], "trim-singles", v)) a.trim_singles = v;
        else if (opt(argv[i], "filter-pairs", v)) a.filter_pairs = v;
        else if (opt(argv[i], "filter-interleaved", v)) a.filter_interleaved = true;
        else if (opt(argv[i], "trim-interleaved", v)) a.trim_interleaved = true;
        else if (opt(argv[i], "pair-names", v)) a.pair_names = true;
        else if (opt(argv[i], "read-stats", v)) { a.read_stats = v; if (v.empty()) return usage(); }
        else if (opt(argv[i], "devices", v)) {
            for (size_t at = 0; at < v.size();) {
                const size_t c = v.find(',', at);
                a.devices.push_back(atoi(v.substr(at, c == std::string::npos ? c : c - at).c_str()));
                if (c == std::string::npos) break;
                at = c + 1;
            }
        }
        else if (opt(argv[i], "help", v)) return usage();
        else if (argv[i][0] == '-') { std::cerr << "unknown option " << argv[i] << std::endl; return usage(); }
    }
    std::transform(a.mode.begin(), a.mode.end(), a.mode.begin(), ::toupper);
    if (!a.normalize.empty() || a.normalize_opts) {   // what the normalization refuses, before anything is read
        std::string why;
        if (a.normalize.empty()) why = "--normalize-cutoff and --normalize-round need --normalize=OUT";
        else if (a.input_path.empty()) why = "--normalize needs --input=FILE: it counts the input's reads while it picks them";
        else if (a.check) why = "--normalize does not go with --check: the reference's count file holds the k-mers of every read";
        else if (a.gpus > 1) why = "--normalize runs on one GPU only: a read is judged against the reads kept before it, and each GPU of a --gpus " + std::to_string(a.gpus) + " run sees a share of them";
        else if (a.min_count == 2) why = "--normalize does not go with --min-count=2: normalization inserts by the atomic path, without the prefilter";
        else if (a.l_auto || a.estimate) why = "--normalize does not go with --l=auto or --estimate: the sketch sizes the table for the k-mers of every read, not of the kept ones";
        else if (is_wrapped(a)) why = "--normalize does not read --format=fasta-wrapped: a wrapped record has no single sequence line to judge";
        else if (a.input_path.find(',') != std::string::npos || a.filter_interleaved || a.trim_interleaved ||
                 a.filter_input.find(',') != std::string::npos || a.trim_input.find(',') != std::string::npos)
            why = "--normalize does not go with paired options (two files in --input, --filter-input or --trim-input, or an interleaved one): mates are not judged together yet";
        if (!why.empty()) {
            std::cerr << why << std::endl;
            return usage();
        }
        a.group = false;   // --gpus=1: the one table of this process
    }
    if (a.l_auto || a.estimate) {   // what the table sizing refuses, before anything is read
        const std::string o = a.estimate ? "--estimate" : "--l=auto";
        std::string why;
        if (a.estimate && !a.given_k) why = "--estimate needs --k=K: the number of distinct k-mers depends on it";
        else if (a.input_path.empty()) why = o + " needs --input=FILE: it sketches the k-mers of the input";
        else if (a.gpus > 1) why = o + " runs on one GPU only: the tables of a --gpus " + std::to_string(a.gpus) + " run are not sized by a sketch yet";
        else if (!a.load.empty() || !a.with.empty())
            why = o + " does not go with --load or --with: a database brings k-mers the sketch of --input has not seen";
        else if (is_wrapped(a)) why = o + " does not read --format=fasta-wrapped: wrapped FASTA has no sketch yet";
        else if (!(a.load_factor > 0.0 && a.load_factor <= 0.9)) why = "--load-factor is the load of the table " + o + " aims at: above 0, at most 0.9";
        if (!why.empty()) {
            std::cerr << why << std::endl;
            return usage();
        }
        a.group = false;   // --gpus=1: the one table of this process
    }
    if (a.min_count == 2) {   // what the two-pass count refuses, before anything is read
        std::string why;
        if (a.input_path.empty()) why = "--min-count=2 needs --input=FILE: it reads the input twice";
        else if (a.gpus > 1) why = "--min-count=2 runs on one GPU only: each GPU of a --gpus " + std::to_string(a.gpus) + " run sees a share of the reads, and a k-mer's two occurrences may lie in two shares";
        else if (is_wrapped(a)) why = "--min-count=2 does not read --format=fasta-wrapped: the prefilter reads FASTQ or two-line FASTA records";
        else if (a.check) why = "--min-count=2 does not go with --check: the reference's count file holds the k-mers seen once";
        else if (!a.load.empty()) why = "--min-count=2 does not go with --load: a database's k-mers were never shown to the prefilter";
        else if (a.l_auto || a.estimate) why = "--min-count=2 does not go with --l=auto or --estimate: the sketch sizes the table for all k-mers, those seen once included";
        if (!why.empty()) {
            std::cerr << why << std::endl;
            return usage();
        }
        a.group = false;   // --gpus=1: the one table of this process
    } else if (a.prefilter_bits) {
        std::cerr << "--prefilter-bits needs --min-count=2" << std::endl;
        return usage();
    }
    if (a.input_path.empty() && a.load.empty()) return usage();
    // --load: the first database sets k, l, s and the seed unless they are given; every one must match the counting mode
    int overflow_l = 0;
    for (size_t i = 0; i < a.load.size(); ++i) {
        tsx_hip_db_info d;
        try {
            d = TSXHashMapHIP::databaseInfo(a.load[i]);
        } catch (const TSXException &e) {
            std::cerr << "--load=" << a.load[i] << ": " << e.what() << std::endl;
            return 3;
        }
        if (i == 0) {
            if (!a.given_k) a.k = d.k;
            if (!a.given_l) a.l = d.l;
            if (!a.given_s) a.storagebits = d.count_bits;
            if (!a.given_seed) a.seed = d.hash_seed;
            if (a.l == d.l && a.storagebits == d.count_bits) overflow_l = d.overflow_l;
        }
        if (d.k != a.k || (d.canonical != 0) != a.canonical || (d.acgt_only != 0) != a.acgt_only || d.min_qual_char != a.min_qual_char) {
            std::cerr << "--load=" << a.load[i] << " was counted with k=" << d.k << (d.canonical ? " --canonical" : "")
                      << (d.acgt_only ? " --acgt-only" : "");
            if (d.min_qual_char) std::cerr << " --min-qual-char=" << (char)d.min_qual_char;
            std::cerr << "; give the same k, --canonical, --acgt-only and --min-qual-char to load it" << std::endl;
            return 2;
        }
    }
    // table set operations: what the options and the headers of --with already tell, before the GPU is touched
    if (op_index(a.op) == -2 || count_index(a.op_count) < 0) {
        std::cerr << "--op is intersect, union, subtract or diff; --op-count is min, max, sum, left or right" << std::endl;
        return usage();
    }
    if ((!a.op.empty() || a.compare) && a.with.empty()) {
        std::cerr << "--op and --compare need a second table: --with=DB[,DB2,...]" << std::endl;
        return usage();
    }
    if ((!a.joint_histo.empty() || a.joint_opts) && a.with.empty()) {
        std::cerr << "--joint-histo needs a second table: --with=DB[,DB2,...]" << std::endl;
        return usage();
    }
    if (a.joint_opts && a.joint_histo.empty()) {
        std::cerr << "--joint-max-a, --joint-max-b and --joint-format go with --joint-histo=FILE" << std::endl;
        return usage();
    }
    if (a.het_opts && a.het_histo.empty() && a.het_pairs.empty()) {
        std::cerr << "--het-max, --het-format, --het-lower, --het-upper and --het-mode go with --het-histo=FILE or --het-pairs=FILE" << std::endl;
        return usage();
    }
    if (!a.het_histo.empty() || !a.het_pairs.empty()) {
        if (a.gpus > 1) {
            std::cerr << "--het-histo and --het-pairs work on one GPU only: a --gpus " << a.gpus << " run keeps one table per GPU, and a"
                      << " k-mer's partners may live on another" << std::endl;
            return usage();
        }
        if (a.het_lower > a.het_upper) { std::cerr << "--het-lower is above --het-upper" << std::endl; return usage(); }
        a.group = false;   // --gpus=1: the one table of this process
    }
    if (!a.joint_histo.empty() && a.gpus > 1) {
        std::cerr << "--joint-histo works on one GPU only: a --gpus " << a.gpus << " run keeps one table per GPU" << std::endl;
        return usage();
    }
    {   // read binning: what the options alone tell
        const bool any_bin = wants_bin(a) || !a.bin_input.empty() || a.bin_opts;
        std::string why;
        if (any_bin && a.with.empty())
            why = "--bin-a, --bin-b, --bin-ambiguous, --bin-none and --bin-stats need a second table: --with=DB[,DB2,...]";
        else if (any_bin && !wants_bin(a))
            why = "--bin-input, --bin-min-hits and --bin-ratio go with --bin-a, --bin-b, --bin-ambiguous, --bin-none or --bin-stats";
        else if (any_bin && a.gpus > 1)
            why = "--bin-a, --bin-b and --bin-stats run on one GPU only: a --gpus " + std::to_string(a.gpus) + " run keeps one table per GPU";
        else if (any_bin && a.bin_input.find(',') != std::string::npos)
            why = "--bin-input takes one file: paired reads are not binned yet";
        else if (any_bin && is_wrapped(a) && (a.bin_input.empty() || a.bin_input == a.input_path))
            why = "--bin-a, --bin-b and --bin-stats do not read wrapped FASTA: give the reads to bin as --bin-input=FILE"
                  " (FASTQ, or FASTA with one sequence line per record)";
        else if (any_bin && a.input_path.empty() && a.bin_input.empty())
            why = "--bin-a, --bin-b and --bin-stats without --input need --bin-input=FILE";
        if (!why.empty()) {
            std::cerr << why << std::endl;
            return usage();
        }
    }
    if (!a.with.empty() && a.op.empty() && !a.compare && a.joint_histo.empty() && !wants_bin(a)) {
        std::cerr << "--with needs --op, --compare, --joint-histo or a --bin-a / --bin-b / --bin-ambiguous / --bin-none / --bin-stats"
                  << " output" << std::endl;
        return usage();
    }
    if (!a.with.empty() && a.gpus > 1) {
        std::cerr << "--with works on one GPU only: a --gpus " << a.gpus << " run keeps one table per GPU" << std::endl;
        return usage();
    }
    if (std::max<uint64_t>(1, a.a_lower) > a.a_upper || std::max<uint64_t>(1, a.b_lower) > a.b_upper) return usage();
    tsx_hip_db_info with_first;
    memset(&with_first, 0, sizeof with_first);
    for (size_t i = 0; i < a.with.size(); ++i) {
        tsx_hip_db_info d;
        try {
            d = TSXHashMapHIP::databaseInfo(a.with[i]);
        } catch (const TSXException &e) {
            std::cerr << "--with=" << a.with[i] << ": " << e.what() << std::endl;
            return 3;
        }
        if (i == 0) with_first = d;
        if (d.k != a.k || (d.canonical != 0) != a.canonical || (d.acgt_only != 0) != a.acgt_only || d.min_qual_char != a.min_qual_char) {
            std::cerr << "--with=" << a.with[i] << " was counted with k=" << d.k << (d.canonical ? " --canonical" : "")
                      << (d.acgt_only ? " --acgt-only" : "");
            if (d.min_qual_char) std::cerr << " --min-qual-char=" << (char)d.min_qual_char;
            std::cerr << "; the first table has k=" << a.k << (a.canonical ? " --canonical" : "") << (a.acgt_only ? " --acgt-only" : "");
            if (a.min_qual_char) std::cerr << " --min-qual-char=" << (char)a.min_qual_char;
            std::cerr << ": both tables of a set operation need the same" << std::endl;
            return 2;
        }
    }

    std::cout << "Running with parameters " << std::endl;
    std::cerr << "K=" << a.k << std::endl;
    if (a.l_auto || a.estimate) std::cerr << "L=auto" << std::endl;
    else std::cerr << "L=" << a.l << std::endl;
    std::cerr << "StorageBits=" << a.storagebits << std::endl;
    std::cerr << "Check=" << (a.check ? "Yes" : "No") << std::endl;
    if (a.canonical) std::cerr << "Canonical=Yes" << std::endl;
    if (a.acgt_only) std::cerr << "AcgtOnly=Yes" << std::endl;
    if (a.min_qual_char) std::cerr << "MinQualChar=" << (char)a.min_qual_char << std::endl;
    std::cerr << "Input=" << a.input_path << std::endl;
    for (const std::string &db : a.load) std::cerr << "Load=" << db << std::endl;
    for (const std::string &db : a.with) std::cerr << "With=" << db << std::endl;
    if (!a.op.empty()) std::cerr << "Op=" << a.op << " OpCount=" << a.op_count << std::endl;
    if (!a.save.empty()) std::cerr << "Save=" << a.save << std::endl;
    std::cerr << "Threads=" << a.threads << std::endl;
    std::cerr << "Mode=" << a.mode << std::endl;
    if (a.mode != "HIP") {
        std::cerr << "This binary implements --mode=HIP only; SERIAL/PTHREAD/OMP/CAS/TSX are the reference's CPU modes."
                  << std::endl;
        return 2;
    }

    if (a.exchange != "merge" && a.exchange != "mini" && a.exchange != "auto") return usage();
    if (a.lower > a.upper || a.histo_max < 1 || a.histo_max > ((uint64_t)1 << 32)) return usage();
    if (a.canonical && a.group && a.exchange == "mini") {
        std::cerr << "--exchange=mini cannot count canonically (its owners are strand-dependent); use --exchange=merge" << std::endl;
        return usage();
    }
    if ((a.acgt_only || a.min_qual_char) && a.group && a.exchange == "mini") {
        std::cerr << "--exchange=mini has no base rule (--acgt-only, --min-qual-char); use --exchange=merge" << std::endl;
        return usage();
    }
    if (a.min_qual_char && is_fasta(a)) {
        std::cerr << "--min-qual-char needs FASTQ input: a FASTA record has no quality line" << std::endl;
        return usage();
    }
    if (wants_medians(a)) {   // what the median forms refuse, before the share rule's checks
        std::string why;
        if (a.filter_median && a.filter_share)
            why = "--filter-median-lower / --filter-median-upper switch --filter to the median rule: they do not go with"
                  " --filter-lower, --filter-upper, --filter-min or --filter-fraction";
        else if (a.filter_median && a.filter.empty()) why = "--filter-median-lower / --filter-median-upper need --filter=OUT";
        else if (a.filter_median && a.filter_median_lower > a.filter_median_upper) why = "--filter-median-lower is above --filter-median-upper";
        else if (filter_paired(a))
            why = "--read-medians and the median rule of --filter do not take paired input (two --filter-input files or"
                  " --filter-interleaved): medians of mate pairs are not built yet";
        else if (a.gpus > 1)
            why = "--read-medians and the median rule of --filter run on one GPU only: every k-mer lives on one rank of a --gpus " +
                  std::to_string(a.gpus) + " run. Count with --gpus=1 (or without --gpus)";
        else if (is_wrapped(a) && (a.filter_input.empty() || a.filter_input == a.input_path))
            why = "--read-medians and the median rule of --filter do not read wrapped FASTA: give the reads as --filter-input=FILE"
                  " (FASTQ, or FASTA with one sequence line per record)";
        if (!why.empty()) {
            std::cerr << why << std::endl;
            return usage();
        }
    }
    if (is_wrapped(a)) {
        if (a.gpus > 1) {
            std::cerr << "--format=fasta-wrapped runs on one GPU only: a --gpus " << a.gpus << " run cuts the text at two-line or"
                      << " four-line records" << std::endl;
            return usage();
        }
        if (a.min_qual_char) {
            std::cerr << "--min-qual-char needs FASTQ input: a FASTA record has no quality line" << std::endl;
            return usage();
        }
        if (wants_queries(a) && (a.filter_input.empty() || a.filter_input == a.input_path)) {
            std::cerr << "--filter and --read-stats do not read wrapped FASTA: give the reads to query as --filter-input=FILE"
                      << " (FASTQ, or FASTA with one sequence line per record)" << std::endl;
            return usage();
        }
        if (wants_trim(a) && (a.trim_input.empty() || a.trim_input == a.input_path)) {
            std::cerr << "--trim and --trim-spans do not read wrapped FASTA: give the reads to trim as --trim-input=FILE"
                      << " (FASTQ, or FASTA with one sequence line per record)" << std::endl;
            return usage();
        }
        a.group = false;   // --gpus=1: the one table of this process
    }
    if (a.filter_pairs != "both" && a.filter_pairs != "any") return usage();
    for (int trim = 0; trim < 2; ++trim) {
        const bool paired = trim ? trim_paired(a) : filter_paired(a);
        const std::string &singles = trim ? a.trim_singles : a.filter_singles;
        std::string why;
        if (paired) why = pairs_refusal(a, trim != 0);
        else if (!singles.empty()) why = std::string(trim ? "--trim-singles" : "--filter-singles") + " needs paired input (R1,R2 or the interleaved form)";
        if (why.empty() && paired && is_wrapped(a))
            for (const std::string &p : split_commas(trim ? a.trim_input : a.filter_input))
                if (p == a.input_path) why = "paired input does not read wrapped FASTA: " + p;
        if (!why.empty()) {
            std::cerr << why << std::endl;
            return usage();
        }
    }
    if (a.gpus < 1 || (a.comm != "rccl" && a.comm != "copy") || (!a.devices.empty() && (int)a.devices.size() != a.gpus)) return usage();
    if (a.filter_lower > a.filter_upper || !(a.filter_fraction >= 0.0 && a.filter_fraction <= 1.0)) return usage();
    if (wants_queries(a) && a.gpus > 1) {
        std::cerr << "--filter and --read-stats run on one GPU only: every k-mer lives on one rank of a --gpus " << a.gpus
                  << " run, and per-rank queries are not combined yet. Count with --gpus=1 (or without --gpus) to filter."
                  << std::endl;
        return usage();
    }
    if (a.trim_lower > a.trim_upper || (a.trim_mode != "longest" && a.trim_mode != "prefix")) return usage();
    if (wants_trim(a) && a.gpus > 1) {
        std::cerr << "--trim and --trim-spans run on one GPU only: every k-mer lives on one rank of a --gpus " << a.gpus
                  << " run, and per-rank spans are not combined yet. Count with --gpus=1 (or without --gpus) to trim."
                  << std::endl;
        return usage();
    }
    if (wants_trim(a) && a.input_path.empty() && a.trim_input.empty()) {
        std::cerr << "--trim and --trim-spans without --input need --trim-input=FILE" << std::endl;
        return usage();
    }
    if ((!a.save.empty() || !a.load.empty()) && a.gpus > 1) {
        std::cerr << "--save and --load work on one GPU only: a --gpus " << a.gpus << " run keeps one table per GPU. Count with"
                  << " --gpus=1 (or without --gpus) to save or load a k-mer database." << std::endl;
        return usage();
    }
    if (!a.load.empty() && a.check) {
        std::cerr << "--check compares the counts with those of --input alone: it cannot follow --load" << std::endl;
        return usage();
    }
    if (wants_queries(a) && a.input_path.empty() && a.filter_input.empty()) {
        std::cerr << "--filter and --read-stats without --input need --filter-input=FILE" << std::endl;
        return usage();
    }
    if ((!a.het_histo.empty() || !a.het_pairs.empty()) && !(a.k & 1)) {
        std::cerr << "--het-histo and --het-pairs need an odd k: a " << a.k << "-mer has no middle base" << std::endl;
        return usage();
    }
    if (!a.save.empty() || !a.load.empty() || !a.with.empty()) a.group = false;   // --gpus=1: the one table of this process
    try {
        if (a.group) return run_group(a);
        std::vector<char> owned;
        const char *text = nullptr;
        size_t n = 0;
        void *map = nullptr;
        bool bgzf = false, loaded = false;
        if (a.l_auto || a.estimate) {   // the text is loaded once: the count below takes it as it is
            if (!load_input(a.input_path, owned, text, n, map, bgzf, true)) {
                std::cerr << "Could not read " << a.input_path << std::endl;
                return 3;
            }
            loaded = true;
            size_input(a, text, n, bgzf);
            if (a.estimate) {
                if (map) munmap(map, n);
                return 0;
            }
        }
        std::cerr << "Creating TSXHashMap HIP" << std::endl;
        TSXHashMapHIP oMap((uint8_t)a.l, (uint32_t)a.storagebits, (uint16_t)a.k, (uint8_t)a.threads, a.seed, a.device, overflow_l);
        if (is_wrapped(a)) std::cerr << "Format=FASTA (wrapped, lines joined)" << std::endl;
        else if (is_fasta(a)) { oMap.setRecordLines(2); std::cerr << "Format=FASTA (2 lines per record)" << std::endl; }
        if (a.canonical) oMap.setCanonical(true);
        if (a.acgt_only || a.min_qual_char) oMap.setBaseRule(a.acgt_only, a.min_qual_char);
        const bool wrapped = is_wrapped(a);
        if (!loaded && !a.input_path.empty() && !load_input(a.input_path, owned, text, n, map, bgzf, true)) {
            std::cerr << "Could not read " << a.input_path << std::endl;
            return 3;
        }
        auto t0 = std::chrono::steady_clock::now();
        for (const std::string &db : a.load) {
            const uint64_t iEntries = oMap.loadDatabase(db);
            std::cerr << "Loaded " << iEntries << " kmers from " << db << std::endl;
        }
        if (a.min_count == 2) {   // pass 1: the input into the prefilter; the count below is pass 2
            const int bits = a.prefilter_bits ? a.prefilter_bits : std::min(38, std::max(12, a.l + 6));
            if (bgzf) {
                try {
                    oMap.prefilterBgzf(text, n, bits);
                } catch (const TSXException &e) {   // (as the count below: without room for the batches, through zlib)
                    if (e.code() != TSX_HIP_ENOMEM) throw;
                    std::cerr << "BGZF on the device: " << e.what() << " -- reading through zlib instead" << std::endl;
                    if (!read_gz(a.input_path, owned)) { std::cerr << "Could not read " << a.input_path << std::endl; return 3; }
                    if (map) munmap(map, n);
                    map = nullptr; text = owned.data(); n = owned.size(); bgzf = false;
                }
            }
            if (!bgzf) oMap.prefilter(text, n, bits);
            oMap.armPrefilter(true);
        }
        if (a.input_path.empty()) {
            // nothing to count: the loaded tables are the result
        } else if (!a.normalize.empty()) {
            if (bgzf) {   // inflated on the device, as the read queries read a BGZF file
                size_t members = 0, tb = 0, got = 0;
                int rc = tsx_hip_bgzf_index_host(text, n, &members, &tb);
                std::vector<char> inflated(tb ? tb : 1);
                if (rc == TSX_HIP_OK) rc = tsx_hip_inflate_bgzf_host(a.device, text, n, inflated.data(), tb, &got);
                if (rc != TSX_HIP_OK) throw TSXException(std::string(tsx_hip_strerror(rc)) + " (" + tsx_hip_last_error() + ")", rc);
                munmap(map, n);
                map = nullptr;
                owned.swap(inflated);
                owned.resize(got);
                text = owned.data();
                n = got;
            }
            const tsx_hip_normalize_totals nt = oMap.normalizeReads(text, n, a.normalize_cutoff, a.normalize_round, a.normalize);
            std::cout << "normalize\t" << nt.records << '\t' << nt.kept << '\t' << nt.kmers_seen << '\t' << nt.kmers_added << '\t'
                      << nt.rounds << std::endl;
            std::cerr << "Normalization kept " << nt.kept << " of " << nt.records << " records (cutoff " << a.normalize_cutoff
                      << ", rounds of " << a.normalize_round << ") in " << a.normalize << std::endl;
        } else if (bgzf) {
            try {
                if (wrapped) oMap.countFastaBgzf(text, n);
                else oMap.countFastqBgzf(text, n);
            } catch (const TSXException &e) {
                // the device path needs two batch-sized text buffers next to the table: without them the input is
                // read the way the reference reads it (zlib on the host) and counted through the staged host path
                if (e.code() != TSX_HIP_ENOMEM) throw;
                std::cerr << "BGZF on the device: " << e.what() << " -- reading through zlib instead" << std::endl;
                oMap.clear();
                for (const std::string &db : a.load) oMap.loadDatabase(db);
                if (!read_gz(a.input_path, owned)) { std::cerr << "Could not read " << a.input_path << std::endl; return 3; }
                if (wrapped) oMap.countFasta(owned.data(), owned.size());
                else oMap.countFastq(owned.data(), owned.size());
            }
        } else if (wrapped) {
            oMap.countFasta(text, n);
        } else {
            oMap.countFastq(text, n);
        }
        double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (map) munmap(map, n);
        if (a.min_count == 2) {
            oMap.armPrefilter(false);
            const tsx_hip_prefilter_totals pt = oMap.prefilterStats();
            std::cout << "prefilter\t" << pt.bits << '\t' << pt.seen << '\t' << pt.seen_again << '\t' << pt.admitted << '\t' << pt.skipped << std::endl;
            std::cerr << "Prefilter: " << pt.skipped << " of " << pt.seen << " k-mer occurrences kept out of the table; filter fill "
                      << pt.set_bits_a << " / 2^" << pt.bits << " and " << pt.set_bits_b << " / 2^" << (pt.bits - 2) << " bits" << std::endl;
        }
        if (a.with.empty()) {
            const int rc = report_and_check(oMap, a, dt);
            if (!wants_queries(a) && !wants_trim(a)) return rc;
            const int rq = run_after(oMap.handle(), a);
            return rc ? rc : rq;
        }
        // --with: B is built like its first database, OUT like A; the result takes A's place from here on
        const int rc = report_and_check(oMap, a, dt, a.op.empty());
        std::cerr << "Creating the second table" << std::endl;
        TSXHashMapHIP oWith((uint8_t)with_first.l, (uint32_t)with_first.count_bits, (uint16_t)a.k, (uint8_t)a.threads,
                            with_first.hash_seed, a.device, with_first.overflow_l);
        if (a.canonical) oWith.setCanonical(true);
        if (a.acgt_only || a.min_qual_char) oWith.setBaseRule(a.acgt_only, a.min_qual_char);
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
        if (a.op.empty()) {
            if (!wants_queries(a) && !wants_trim(a)) return rc;
            const int rq = run_after(oMap.handle(), a);
            return rc ? rc : rq;
        }
        std::cerr << "Creating the result table" << std::endl;
        TSXHashMapHIP oOut((uint8_t)a.l, (uint32_t)a.storagebits, (uint16_t)a.k, (uint8_t)a.threads, a.seed, a.device, overflow_l);
        if (a.canonical) oOut.setCanonical(true);
        if (a.acgt_only || a.min_qual_char) oOut.setBaseRule(a.acgt_only, a.min_qual_char);
        const tsx_hip_combine_rule oRule = {op_index(a.op), count_index(a.op_count), a.a_lower, a.a_upper, a.b_lower, a.b_upper};
        const tsx_hip_combine_stats s = oMap.combine(oWith, oOut, oRule);
        std::cout << a.op << ": " << s.out_entries << " different kmers, count sum " << s.out_count_sum << " (first table "
                  << s.a_in_range << ", second " << s.b_in_range << ", both " << s.both << " in range)" << std::endl;
        save_database(oOut, a);
        write_outputs(oOut, a);
        if (!wants_queries(a) && !wants_trim(a)) return rc;
        const int rq = run_after(oOut.handle(), a);
        return rc ? rc : rq;
    } catch (const TSXException &e) {
        std::cerr << "TSXException: " << e.what() << std::endl;
        return e.code() == TSX_HIP_EFULL ? 42 : 10;  // exit(42): TSXHashMap.h:340-343
    }
}
