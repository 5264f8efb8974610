// cli_options.h -- what the tsxCount command line takes and what it turns down before a table is created: the arguments,
// the usage text, one table of options with the loop that walks it, and the refusals in the order main() asks them.
// To add an option: one row in parse_options, one refusal function (or a line in its feature's), one paragraph in
// usage(), one command line in tests/golden/make_cli_refusals.py ("Adding a command-line option").
#pragma once
#include <algorithm>
#include <cerrno>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "TSXHashMapHIP.h"

struct arguments {
    int k = 14, l = 26, storagebits = 4, threads = 0;  // main.cpp:410-413
    std::string input_path, mode = "HIP", format;   // format: "", "fastq", "fasta" or "fasta-wrapped" ("" = by file name)
    bool check = false, checkabort = false;
    uint64_t seed = 1;
    int device = 0;
    bool group = false;           // --gpus given: the group path, even for one GPU, unless a feature needs the one table (uses_group)
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

// ---- what the options ask for -----------------------------------------------------------------------------------------------

static bool is_wrapped(const arguments &a) { return a.format == "fasta-wrapped"; }   // multi-line FASTA, lines joined on the GPU

// FASTA (two lines per record, FASTXreader<FASTAEntry>) by option or by file name
static bool is_fasta_path(const std::string &path, const std::string &format) {
    std::string stem = path;
    if (stem.size() > 3 && stem.rfind(".gz") == stem.size() - 3) stem.resize(stem.size() - 3);
    auto ends = [&](const char *suf) { const std::string x(suf); return stem.size() >= x.size() && stem.compare(stem.size() - x.size(), x.size(), x) == 0; };
    return format == "fasta" || (format.empty() && (ends(".fa") || ends(".fasta") || ends(".fna")));
}
static bool is_fasta(const arguments &a) { return is_fasta_path(a.input_path, a.format); }

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
static bool wants_queries(const arguments &a) { return !a.filter.empty() || !a.read_stats.empty() || !a.read_medians.empty(); }
static bool wants_medians(const arguments &a) { return !a.read_medians.empty() || a.filter_median; }
static bool wants_trim(const arguments &a) { return !a.trim.empty() || !a.trim_spans.empty(); }
static bool wants_het(const arguments &a) { return !a.het_histo.empty() || !a.het_pairs.empty(); }
static bool wants_bin_reads(const arguments &a) {
    return !a.bin_a.empty() || !a.bin_b.empty() || !a.bin_ambiguous.empty() || !a.bin_none.empty();
}
static bool wants_bin(const arguments &a) { return wants_bin_reads(a) || !a.bin_stats.empty(); }

// --op / --op-count by name: the TSX_HIP_OP_* / TSX_HIP_CNT_* value, -1 for none given, -2 / -1 for an unknown one
static int op_index(const std::string &s) {
    return s.empty() ? -1 : s == "intersect" ? TSX_HIP_OP_INTERSECT : s == "union" ? TSX_HIP_OP_UNION
         : s == "subtract" ? TSX_HIP_OP_SUBTRACT : s == "diff" ? TSX_HIP_OP_DIFF : -2;
}
static int count_index(const std::string &s) {
    return s == "min" ? TSX_HIP_CNT_MIN : s == "max" ? TSX_HIP_CNT_MAX : s == "sum" ? TSX_HIP_CNT_SUM
         : s == "left" ? TSX_HIP_CNT_LEFT : s == "right" ? TSX_HIP_CNT_RIGHT : -1;
}

// Whether the run takes the group path.  --gpus=N does, for N = 1 too (its merge then runs through RCCL with one rank),
// unless a feature needs the one table of this process: the refusals have turned N > 1 down for each of them.  The two
// --exchange=mini refusals ask with behind_exchange_refusals = false: wrapped FASTA, --save, --load and --with take a
// --gpus=1 run off the group path only behind them, so --gpus=1 --canonical --exchange=mini is refused with --save and
// passes with --min-count=2.
static bool uses_group(const arguments &a, bool behind_exchange_refusals = true) {
    if (!a.group) return false;
    if (!a.normalize.empty() || a.l_auto || a.estimate || a.min_count == 2 || wants_het(a)) return false;
    if (!behind_exchange_refusals) return true;
    return !is_wrapped(a) && a.save.empty() && a.load.empty() && a.with.empty();
}

// ---- refusals ---------------------------------------------------------------------------------------------------------------

// Why a command line is turned down.  code 0: it is not; 1: the message (if any), then the usage text; 2 and 3: the
// message alone (a mode or database that does not fit, a file that cannot be read).
struct refusal {
    std::string why;
    int code;
    explicit operator bool() const { return code != 0; }
};
static refusal pass() { return {std::string(), 0}; }
static refusal refuse(const std::string &why = std::string(), int code = 1) { return {why, code}; }
static int report(const refusal &r) {
    if (!r.why.empty()) std::cerr << r.why << std::endl;
    return r.code == 1 ? usage() : r.code;
}

// ---- the options ------------------------------------------------------------------------------------------------------------

enum option_kind {
    FLAG,         // bool: true, whatever value comes with it (--check=anything)
    STRING,       // std::string
    NONEMPTY,     // std::string that must not be empty
    INT,          // int through atoi, uint64_t through strtoull, double through atof: junk reads as 0, nothing is refused
    U64,
    DOUBLE,
    STRICT_U64,   // uint64_t, digits only, lo <= x <= hi
    WORD,         // std::string, one of `words`
    STRING_LIST,  // std::vector<std::string>, comma-separated and appended, no element empty
    INT_LIST,     // std::vector<int>, comma-separated and appended, each through atoi
    CUSTOM        // the option's own function
};
struct option {
    const char *name;
    option_kind kind;
    void *to;               // where the value goes: the type its kind names
    bool *given;            // raised when the value is taken (nullptr: nothing to raise)
    uint64_t lo, hi;        // STRICT_U64
    bool refuse_overflow;   // STRICT_U64: a value above 2^64 - 1 is refused (else strtoull's 2^64 - 1 is taken)
    const char *words;      // WORD: "this,that"
    const char *message;    // what a refused value prints in front of the usage text ("": nothing)
    bool (*custom)(const std::string &v, arguments &a, std::string &why);   // CUSTOM: false refuses, with `why` (preset to message)
};
static option flag(const char *name, bool &to) { return {name, FLAG, &to, nullptr, 0, 0, false, "", "", nullptr}; }
static option text(const char *name, std::string &to) { return {name, STRING, &to, nullptr, 0, 0, false, "", "", nullptr}; }
static option nonempty(const char *name, std::string &to) { return {name, NONEMPTY, &to, nullptr, 0, 0, false, "", "", nullptr}; }
static option lenient(const char *name, int &to, bool *given = nullptr) { return {name, INT, &to, given, 0, 0, false, "", "", nullptr}; }
static option lenient(const char *name, uint64_t &to, bool *given = nullptr) { return {name, U64, &to, given, 0, 0, false, "", "", nullptr}; }
static option lenient(const char *name, double &to, bool *given = nullptr) { return {name, DOUBLE, &to, given, 0, 0, false, "", "", nullptr}; }
static option strict(const char *name, uint64_t &to, bool *given, uint64_t lo, uint64_t hi, bool refuse_overflow, const char *message) {
    return {name, STRICT_U64, &to, given, lo, hi, refuse_overflow, "", message, nullptr};
}
static option word(const char *name, std::string &to, bool *given, const char *words, const char *message) {
    return {name, WORD, &to, given, 0, 0, false, words, message, nullptr};
}
static option list(const char *name, std::vector<std::string> &to) { return {name, STRING_LIST, &to, nullptr, 0, 0, false, "", "", nullptr}; }
static option list(const char *name, std::vector<int> &to) { return {name, INT_LIST, &to, nullptr, 0, 0, false, "", "", nullptr}; }
static option custom(const char *name, bool (*fn)(const std::string &, arguments &, std::string &), const char *message = "") {
    return {name, CUSTOM, nullptr, nullptr, 0, 0, false, "", message, fn};
}

// the options that are their own kind
static bool take_l(const std::string &v, arguments &a, std::string &) {
    if (v == "auto") a.l_auto = true;
    else { a.l = atoi(v.c_str()); a.given_l = true; a.l_auto = false; }
    return true;
}
static bool take_min_count(const std::string &v, arguments &a, std::string &) {
    if (v != "1" && v != "2") return false;
    a.min_count = atoi(v.c_str());
    return true;
}
static bool take_prefilter_bits(const std::string &v, arguments &a, std::string &) {   // (signed: a '-' reads as a number below 12)
    char *end = nullptr;
    const long b = strtol(v.c_str(), &end, 10);
    if (v.empty() || *end || b < 12 || b > 38) return false;
    a.prefilter_bits = (int)b;
    return true;
}
static bool take_min_qual_char(const std::string &v, arguments &a, std::string &) {
    if (v.size() != 1) return false;
    a.min_qual_char = (unsigned char)v[0];
    return true;
}
// --bin-ratio: digits[.digits], 1 .. 1000, in thousandths (the decimals behind the third are dropped)
static bool take_bin_ratio(const std::string &v, arguments &a, std::string &why) {
    why = "--bin-ratio takes a decimal 1 .. 1000 (three places are kept), not '" + v + "'";
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
    a.bin_ratio_milli = (uint32_t)m;
    a.bin_opts = true;
    return true;
}
static bool take_help(const std::string &, arguments &, std::string &) { return false; }

// One value into one option; false when the option turns it down (`why` then holds what to say, or nothing).
static bool take(const option &o, const std::string &v, arguments &a, std::string &why) {
    why = o.message;
    switch (o.kind) {
    case FLAG: *(bool *)o.to = true; break;
    case STRING: *(std::string *)o.to = v; break;
    case NONEMPTY:
        if (v.empty()) return false;
        *(std::string *)o.to = v;
        break;
    case INT: *(int *)o.to = atoi(v.c_str()); break;
    case U64: *(uint64_t *)o.to = strtoull(v.c_str(), nullptr, 10); break;
    case DOUBLE: *(double *)o.to = atof(v.c_str()); break;
    case STRICT_U64: {
        char *end = nullptr;
        errno = 0;
        const uint64_t x = strtoull(v.c_str(), &end, 10);
        if (v.empty() || *end || (o.refuse_overflow && errno) || v[0] == '-' || x < o.lo || x > o.hi) return false;
        *(uint64_t *)o.to = x;
        break;
    }
    case WORD: {
        const std::vector<std::string> words = split_commas(std::string(o.words));
        if (std::find(words.begin(), words.end(), v) == words.end()) return false;
        *(std::string *)o.to = v;
        break;
    }
    case STRING_LIST:
        for (const std::string &one : split_commas(v)) {
            if (one.empty()) return false;
            ((std::vector<std::string> *)o.to)->push_back(one);
        }
        break;
    case INT_LIST:   // (an empty value and the empty tail behind a last comma name no device)
        for (size_t at = 0; at < v.size();) {
            const size_t c = v.find(',', at);
            ((std::vector<int> *)o.to)->push_back(atoi(v.substr(at, c == std::string::npos ? c : c - at).c_str()));
            if (c == std::string::npos) break;
            at = c + 1;
        }
        break;
    case CUSTOM:
        if (!o.custom(v, a, why)) return false;
        break;
    }
    if (o.given) *o.given = true;
    return true;
}

// argv into `a`: --name or --name=value, in any order, a later value over an earlier one; a word without a leading '-'
// is passed over (main.cpp takes its options the same way).
static refusal parse_options(int argc, char *argv[], arguments &a) {
    const uint64_t MAX = UINT64_MAX;
    // (H + 2)^2 <= 2^24 cells for either side of a count matrix: H <= 4094
    const char *joint_max = "--joint-max-a / --joint-max-b take the largest count with a bin of its own: a number 1 .. 4094";
    const char *het_range = "--het-lower / --het-upper take a count: a number 0 .. 2^64 - 1";
    const option table[] = {
        lenient("k", a.k, &a.given_k),
        custom("l", take_l),
        flag("estimate", a.estimate),
        lenient("load-factor", a.load_factor),
        custom("min-count", take_min_count, "--min-count takes 1 (count every k-mer) or 2 (keep k-mers seen once out of the table)"),
        custom("prefilter-bits", take_prefilter_bits, "--prefilter-bits is the log2 of the prefilter's size in bits: a number 12 .. 38"),
        lenient("s", a.storagebits, &a.given_s),
        lenient("threads", a.threads),
        text("input", a.input_path),
        text("mode", a.mode),
        flag("check", a.check),
        flag("checkabort", a.checkabort),
        lenient("seed", a.seed, &a.given_seed),
        nonempty("save", a.save),
        list("load", a.load),
        list("with", a.with),
        nonempty("op", a.op),
        text("op-count", a.op_count),
        lenient("a-lower", a.a_lower),
        lenient("a-upper", a.a_upper),
        lenient("b-lower", a.b_lower),
        lenient("b-upper", a.b_upper),
        flag("compare", a.compare),
        nonempty("joint-histo", a.joint_histo),
        strict("joint-max-a", a.joint_max_a, &a.joint_opts, 1, 4094, true, joint_max),
        strict("joint-max-b", a.joint_max_b, &a.joint_opts, 1, 4094, true, joint_max),
        word("joint-format", a.joint_format, &a.joint_opts, "sparse,matrix", "--joint-format is sparse or matrix"),
        nonempty("bin-a", a.bin_a),
        nonempty("bin-b", a.bin_b),
        nonempty("bin-ambiguous", a.bin_ambiguous),
        nonempty("bin-none", a.bin_none),
        nonempty("bin-input", a.bin_input),
        nonempty("bin-stats", a.bin_stats),
        strict("bin-min-hits", a.bin_min_hits, &a.bin_opts, 0, MAX, true, "--bin-min-hits takes a number"),
        custom("bin-ratio", take_bin_ratio),
        nonempty("het-histo", a.het_histo),
        nonempty("het-pairs", a.het_pairs),
        strict("het-max", a.het_max, &a.het_opts, 1, 4094, true, "--het-max takes the largest count with a bin of its own: a number 1 .. 4094"),
        word("het-format", a.het_format, &a.het_opts, "sparse,matrix", "--het-format is sparse or matrix"),
        word("het-mode", a.het_mode, &a.het_opts, "unique,all", "--het-mode is unique or all"),
        strict("het-lower", a.het_lower, &a.het_opts, 0, MAX, true, het_range),
        strict("het-upper", a.het_upper, &a.het_opts, 0, MAX, true, het_range),
        text("format", a.format),
        lenient("device", a.device),
        lenient("gpus", a.gpus, &a.group),
        text("comm", a.comm),
        text("exchange", a.exchange),
        flag("canonical", a.canonical),
        flag("acgt-only", a.acgt_only),
        custom("min-qual-char", take_min_qual_char, "--min-qual-char takes one character (e.g. --min-qual-char=5)"),
        text("output", a.output),
        lenient("lower", a.lower),
        lenient("upper", a.upper),
        text("histo", a.histo),
        lenient("histo-max", a.histo_max),
        nonempty("filter", a.filter),
        text("filter-input", a.filter_input),
        lenient("filter-lower", a.filter_lower, &a.filter_share),
        lenient("filter-upper", a.filter_upper, &a.filter_share),
        lenient("filter-min", a.filter_min, &a.filter_share),
        lenient("filter-fraction", a.filter_fraction, &a.filter_share),
        lenient("filter-median-lower", a.filter_median_lower, &a.filter_median),
        lenient("filter-median-upper", a.filter_median_upper, &a.filter_median),
        nonempty("read-medians", a.read_medians),
        nonempty("normalize", a.normalize),
        strict("normalize-cutoff", a.normalize_cutoff, &a.normalize_opts, 0, MAX, false, "--normalize-cutoff takes a count, 0 or more"),
        strict("normalize-round", a.normalize_round, &a.normalize_opts, 1, MAX, false, "--normalize-round takes a number of records, 1 or more"),
        flag("filter-invert", a.filter_invert),
        nonempty("trim", a.trim),
        nonempty("trim-spans", a.trim_spans),
        text("trim-input", a.trim_input),
        lenient("trim-lower", a.trim_lower),
        lenient("trim-upper", a.trim_upper),
        text("trim-mode", a.trim_mode),
        lenient("trim-min-len", a.trim_min_len),
        text("filter-singles", a.filter_singles),
        text("trim-singles", a.trim_singles),
        text("filter-pairs", a.filter_pairs),
        flag("filter-interleaved", a.filter_interleaved),
        flag("trim-interleaved", a.trim_interleaved),
        flag("pair-names", a.pair_names),
        nonempty("read-stats", a.read_stats),
        list("devices", a.devices),
        custom("help", take_help),
    };
    for (int i = 1; i < argc; ++i) {
        const std::string arg(argv[i]);
        if (arg.rfind("--", 0) != 0) {
            if (arg[0] == '-') return refuse("unknown option " + arg);
            continue;
        }
        const size_t eq = arg.find('=');
        const std::string name = arg.substr(2, eq == std::string::npos ? eq : eq - 2);
        const std::string v = eq == std::string::npos ? std::string() : arg.substr(eq + 1);
        const option *o = std::find_if(std::begin(table), std::end(table), [&](const option &x) { return name == x.name; });
        if (o == std::end(table)) return refuse("unknown option " + arg);
        std::string why;
        if (!take(*o, v, a, why)) return refuse(why);
    }
    std::transform(a.mode.begin(), a.mode.end(), a.mode.begin(), ::toupper);
    return pass();
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

// -- from the options alone, before a file is opened

static refusal refuse_normalize(const arguments &a) {
    if (a.normalize.empty() && !a.normalize_opts) return pass();
    if (a.normalize.empty()) return refuse("--normalize-cutoff and --normalize-round need --normalize=OUT");
    if (a.input_path.empty()) return refuse("--normalize needs --input=FILE: it counts the input's reads while it picks them");
    if (a.check) return refuse("--normalize does not go with --check: the reference's count file holds the k-mers of every read");
    if (a.gpus > 1) return refuse("--normalize runs on one GPU only: a read is judged against the reads kept before it, and each GPU of a --gpus " + std::to_string(a.gpus) + " run sees a share of them");
    if (a.min_count == 2) return refuse("--normalize does not go with --min-count=2: normalization inserts by the atomic path, without the prefilter");
    if (a.l_auto || a.estimate) return refuse("--normalize does not go with --l=auto or --estimate: the sketch sizes the table for the k-mers of every read, not of the kept ones");
    if (is_wrapped(a)) return refuse("--normalize does not read --format=fasta-wrapped: a wrapped record has no single sequence line to judge");
    if (a.input_path.find(',') != std::string::npos || filter_paired(a) || trim_paired(a))
        return refuse("--normalize does not go with paired options (two files in --input, --filter-input or --trim-input, or an interleaved one): mates are not judged together yet");
    return pass();
}

static refusal refuse_sizing(const arguments &a) {   // --l=auto and --estimate
    if (!a.l_auto && !a.estimate) return pass();
    const std::string o = a.estimate ? "--estimate" : "--l=auto";
    if (a.estimate && !a.given_k) return refuse("--estimate needs --k=K: the number of distinct k-mers depends on it");
    if (a.input_path.empty()) return refuse(o + " needs --input=FILE: it sketches the k-mers of the input");
    if (a.gpus > 1) return refuse(o + " runs on one GPU only: the tables of a --gpus " + std::to_string(a.gpus) + " run are not sized by a sketch yet");
    if (!a.load.empty() || !a.with.empty())
        return refuse(o + " does not go with --load or --with: a database brings k-mers the sketch of --input has not seen");
    if (is_wrapped(a)) return refuse(o + " does not read --format=fasta-wrapped: wrapped FASTA has no sketch yet");
    if (!(a.load_factor > 0.0 && a.load_factor <= 0.9)) return refuse("--load-factor is the load of the table " + o + " aims at: above 0, at most 0.9");
    return pass();
}

static refusal refuse_min_count(const arguments &a) {   // the two-pass count
    if (a.min_count != 2) return a.prefilter_bits ? refuse("--prefilter-bits needs --min-count=2") : pass();
    if (a.input_path.empty()) return refuse("--min-count=2 needs --input=FILE: it reads the input twice");
    if (a.gpus > 1) return refuse("--min-count=2 runs on one GPU only: each GPU of a --gpus " + std::to_string(a.gpus) + " run sees a share of the reads, and a k-mer's two occurrences may lie in two shares");
    if (is_wrapped(a)) return refuse("--min-count=2 does not read --format=fasta-wrapped: the prefilter reads FASTQ or two-line FASTA records");
    if (a.check) return refuse("--min-count=2 does not go with --check: the reference's count file holds the k-mers seen once");
    if (!a.load.empty()) return refuse("--min-count=2 does not go with --load: a database's k-mers were never shown to the prefilter");
    if (a.l_auto || a.estimate) return refuse("--min-count=2 does not go with --l=auto or --estimate: the sketch sizes the table for all k-mers, those seen once included");
    return pass();
}

static refusal refuse_nothing_to_count(const arguments &a) { return a.input_path.empty() && a.load.empty() ? refuse() : pass(); }

// -- the second table and what reads the table: what the options and the headers of --load tell

static refusal refuse_set_operation(const arguments &a) {
    if (op_index(a.op) == -2 || count_index(a.op_count) < 0)
        return refuse("--op is intersect, union, subtract or diff; --op-count is min, max, sum, left or right");
    if ((!a.op.empty() || a.compare) && a.with.empty()) return refuse("--op and --compare need a second table: --with=DB[,DB2,...]");
    return pass();
}

static refusal refuse_joint_options(const arguments &a) {
    if ((!a.joint_histo.empty() || a.joint_opts) && a.with.empty()) return refuse("--joint-histo needs a second table: --with=DB[,DB2,...]");
    if (a.joint_opts && a.joint_histo.empty()) return refuse("--joint-max-a, --joint-max-b and --joint-format go with --joint-histo=FILE");
    return pass();
}

static refusal refuse_het(const arguments &a) {
    if (a.het_opts && !wants_het(a))
        return refuse("--het-max, --het-format, --het-lower, --het-upper and --het-mode go with --het-histo=FILE or --het-pairs=FILE");
    if (!wants_het(a)) return pass();
    if (a.gpus > 1)
        return refuse("--het-histo and --het-pairs work on one GPU only: a --gpus " + std::to_string(a.gpus) + " run keeps one table per GPU, and a"
                      " k-mer's partners may live on another");
    if (a.het_lower > a.het_upper) return refuse("--het-lower is above --het-upper");
    return pass();
}

static refusal refuse_joint_group(const arguments &a) {
    if (!a.joint_histo.empty() && a.gpus > 1)
        return refuse("--joint-histo works on one GPU only: a --gpus " + std::to_string(a.gpus) + " run keeps one table per GPU");
    return pass();
}

static refusal refuse_bin(const arguments &a) {   // read binning: what the options alone tell
    if (!wants_bin(a) && a.bin_input.empty() && !a.bin_opts) return pass();
    if (a.with.empty()) return refuse("--bin-a, --bin-b, --bin-ambiguous, --bin-none and --bin-stats need a second table: --with=DB[,DB2,...]");
    if (!wants_bin(a)) return refuse("--bin-input, --bin-min-hits and --bin-ratio go with --bin-a, --bin-b, --bin-ambiguous, --bin-none or --bin-stats");
    if (a.gpus > 1) return refuse("--bin-a, --bin-b and --bin-stats run on one GPU only: a --gpus " + std::to_string(a.gpus) + " run keeps one table per GPU");
    if (a.bin_input.find(',') != std::string::npos) return refuse("--bin-input takes one file: paired reads are not binned yet");
    if (is_wrapped(a) && (a.bin_input.empty() || a.bin_input == a.input_path))
        return refuse("--bin-a, --bin-b and --bin-stats do not read wrapped FASTA: give the reads to bin as --bin-input=FILE"
                      " (FASTQ, or FASTA with one sequence line per record)");
    if (a.input_path.empty() && a.bin_input.empty()) return refuse("--bin-a, --bin-b and --bin-stats without --input need --bin-input=FILE");
    return pass();
}

static refusal refuse_with(const arguments &a) {
    if (!a.with.empty() && a.op.empty() && !a.compare && a.joint_histo.empty() && !wants_bin(a))
        return refuse("--with needs --op, --compare, --joint-histo or a --bin-a / --bin-b / --bin-ambiguous / --bin-none / --bin-stats"
                      " output");
    if (!a.with.empty() && a.gpus > 1)
        return refuse("--with works on one GPU only: a --gpus " + std::to_string(a.gpus) + " run keeps one table per GPU");
    if (std::max<uint64_t>(1, a.a_lower) > a.a_upper || std::max<uint64_t>(1, a.b_lower) > a.b_upper) return refuse();
    return pass();
}

// -- behind the "Running with parameters" banner

static refusal refuse_mode(const arguments &a) {
    if (a.mode == "HIP") return pass();
    return refuse("This binary implements --mode=HIP only; SERIAL/PTHREAD/OMP/CAS/TSX are the reference's CPU modes.", 2);
}

static refusal refuse_count_options(const arguments &a) {
    if (a.exchange != "merge" && a.exchange != "mini" && a.exchange != "auto") return refuse();
    if (a.lower > a.upper || a.histo_max < 1 || a.histo_max > ((uint64_t)1 << 32)) return refuse();
    if (a.canonical && uses_group(a, false) && a.exchange == "mini")
        return refuse("--exchange=mini cannot count canonically (its owners are strand-dependent); use --exchange=merge");
    if ((a.acgt_only || a.min_qual_char) && uses_group(a, false) && a.exchange == "mini")
        return refuse("--exchange=mini has no base rule (--acgt-only, --min-qual-char); use --exchange=merge");
    if (a.min_qual_char && is_fasta(a)) return refuse("--min-qual-char needs FASTQ input: a FASTA record has no quality line");
    return pass();
}

static refusal refuse_medians(const arguments &a) {   // what the median forms refuse, before the share rule's checks
    if (!wants_medians(a)) return pass();
    if (a.filter_median && a.filter_share)
        return refuse("--filter-median-lower / --filter-median-upper switch --filter to the median rule: they do not go with"
                      " --filter-lower, --filter-upper, --filter-min or --filter-fraction");
    if (a.filter_median && a.filter.empty()) return refuse("--filter-median-lower / --filter-median-upper need --filter=OUT");
    if (a.filter_median && a.filter_median_lower > a.filter_median_upper) return refuse("--filter-median-lower is above --filter-median-upper");
    if (filter_paired(a))
        return refuse("--read-medians and the median rule of --filter do not take paired input (two --filter-input files or"
                      " --filter-interleaved): medians of mate pairs are not built yet");
    if (a.gpus > 1)
        return refuse("--read-medians and the median rule of --filter run on one GPU only: every k-mer lives on one rank of a --gpus " +
                      std::to_string(a.gpus) + " run. Count with --gpus=1 (or without --gpus)");
    if (is_wrapped(a) && (a.filter_input.empty() || a.filter_input == a.input_path))
        return refuse("--read-medians and the median rule of --filter do not read wrapped FASTA: give the reads as --filter-input=FILE"
                      " (FASTQ, or FASTA with one sequence line per record)");
    return pass();
}

static refusal refuse_wrapped(const arguments &a) {
    if (!is_wrapped(a)) return pass();
    if (a.gpus > 1)
        return refuse("--format=fasta-wrapped runs on one GPU only: a --gpus " + std::to_string(a.gpus) + " run cuts the text at two-line or"
                      " four-line records");
    if (a.min_qual_char) return refuse("--min-qual-char needs FASTQ input: a FASTA record has no quality line");
    if (wants_queries(a) && (a.filter_input.empty() || a.filter_input == a.input_path))
        return refuse("--filter and --read-stats do not read wrapped FASTA: give the reads to query as --filter-input=FILE"
                      " (FASTQ, or FASTA with one sequence line per record)");
    if (wants_trim(a) && (a.trim_input.empty() || a.trim_input == a.input_path))
        return refuse("--trim and --trim-spans do not read wrapped FASTA: give the reads to trim as --trim-input=FILE"
                      " (FASTQ, or FASTA with one sequence line per record)");
    return pass();
}

static refusal refuse_pairs(const arguments &a) {   // the filter's paired form, then the trim's
    if (a.filter_pairs != "both" && a.filter_pairs != "any") return refuse();
    for (int trim = 0; trim < 2; ++trim) {
        const bool paired = trim ? trim_paired(a) : filter_paired(a);
        const std::string &singles = trim ? a.trim_singles : a.filter_singles;
        std::string why;
        if (paired) why = pairs_refusal(a, trim != 0);
        else if (!singles.empty()) why = std::string(trim ? "--trim-singles" : "--filter-singles") + " needs paired input (R1,R2 or the interleaved form)";
        if (why.empty() && paired && is_wrapped(a))
            for (const std::string &p : split_commas(trim ? a.trim_input : a.filter_input))
                if (p == a.input_path) why = "paired input does not read wrapped FASTA: " + p;
        if (!why.empty()) return refuse(why);
    }
    return pass();
}

static refusal refuse_group_options(const arguments &a) {
    if (a.gpus < 1 || (a.comm != "rccl" && a.comm != "copy") || (!a.devices.empty() && (int)a.devices.size() != a.gpus)) return refuse();
    return pass();
}

static refusal refuse_queries(const arguments &a) {
    if (a.filter_lower > a.filter_upper || !(a.filter_fraction >= 0.0 && a.filter_fraction <= 1.0)) return refuse();
    if (wants_queries(a) && a.gpus > 1)
        return refuse("--filter and --read-stats run on one GPU only: every k-mer lives on one rank of a --gpus " + std::to_string(a.gpus) +
                      " run, and per-rank queries are not combined yet. Count with --gpus=1 (or without --gpus) to filter.");
    return pass();
}

static refusal refuse_trim(const arguments &a) {
    if (a.trim_lower > a.trim_upper || (a.trim_mode != "longest" && a.trim_mode != "prefix")) return refuse();
    if (wants_trim(a) && a.gpus > 1)
        return refuse("--trim and --trim-spans run on one GPU only: every k-mer lives on one rank of a --gpus " + std::to_string(a.gpus) +
                      " run, and per-rank spans are not combined yet. Count with --gpus=1 (or without --gpus) to trim.");
    if (wants_trim(a) && a.input_path.empty() && a.trim_input.empty()) return refuse("--trim and --trim-spans without --input need --trim-input=FILE");
    return pass();
}

static refusal refuse_database(const arguments &a) {
    if ((!a.save.empty() || !a.load.empty()) && a.gpus > 1)
        return refuse("--save and --load work on one GPU only: a --gpus " + std::to_string(a.gpus) + " run keeps one table per GPU. Count with"
                      " --gpus=1 (or without --gpus) to save or load a k-mer database.");
    if (!a.load.empty() && a.check) return refuse("--check compares the counts with those of --input alone: it cannot follow --load");
    return pass();
}

static refusal refuse_without_input(const arguments &a) {
    if (wants_queries(a) && a.input_path.empty() && a.filter_input.empty()) return refuse("--filter and --read-stats without --input need --filter-input=FILE");
    return pass();
}

static refusal refuse_het_even_k(const arguments &a) {
    if (wants_het(a) && !(a.k & 1))
        return refuse("--het-histo and --het-pairs need an odd k: a " + std::to_string(a.k) + "-mer has no middle base");
    return pass();
}

// The order they are asked in: the first one that speaks ends the run.  --load's headers are read behind the first list
// (they may set k, l, s and the seed), --with's behind the second, and the banner is printed in front of the third.
typedef refusal (*refusal_fn)(const arguments &);
static const refusal_fn REFUSE_FROM_OPTIONS[] = {refuse_normalize, refuse_sizing, refuse_min_count, refuse_nothing_to_count};
static const refusal_fn REFUSE_OF_TABLES[] = {refuse_set_operation, refuse_joint_options, refuse_het, refuse_joint_group, refuse_bin, refuse_with};
static const refusal_fn REFUSE_BEHIND_BANNER[] = {refuse_mode, refuse_count_options, refuse_medians, refuse_wrapped, refuse_pairs,
                                                  refuse_group_options, refuse_queries, refuse_trim, refuse_database,
                                                  refuse_without_input, refuse_het_even_k};
template <size_t N>
static refusal first_refusal(const refusal_fn (&list)[N], const arguments &a) {
    for (const refusal_fn f : list) {
        const refusal r = f(a);
        if (r) return r;
    }
    return pass();
}

// ---- database headers ---------------------------------------------------------------------------------------------------------

// What the headers of --load and --with leave for the run: the overflow array of the first --load database where the
// table keeps its shape, and the first --with header, which the second table is built like.
struct db_headers {
    int overflow_l = 0;
    tsx_hip_db_info with_first;
    db_headers() { memset(&with_first, 0, sizeof with_first); }
};

static std::string counting_mode_words(int k, bool canonical, bool acgt_only, int min_qual_char) {
    std::string s = "k=" + std::to_string(k) + (canonical ? " --canonical" : "") + (acgt_only ? " --acgt-only" : "");
    if (min_qual_char) s += std::string(" --min-qual-char=") + (char)min_qual_char;
    return s;
}

// The headers of --load (with = false) or --with, before the GPU is touched: every database must be readable and match
// the counting mode.  The first --load database sets k, l, s and the seed unless they are given.
static refusal read_headers(bool with, arguments &a, db_headers &h) {
    const std::vector<std::string> &paths = with ? a.with : a.load;
    const std::string o = with ? "--with=" : "--load=";
    for (size_t i = 0; i < paths.size(); ++i) {
        tsx_hip_db_info d;
        try {
            d = TSXHashMapHIP::databaseInfo(paths[i]);
        } catch (const TSXException &e) {
            return refuse(o + paths[i] + ": " + e.what(), 3);
        }
        if (i == 0 && with) h.with_first = d;
        if (i == 0 && !with) {
            if (!a.given_k) a.k = d.k;
            if (!a.given_l) a.l = d.l;
            if (!a.given_s) a.storagebits = d.count_bits;
            if (!a.given_seed) a.seed = d.hash_seed;
            if (a.l == d.l && a.storagebits == d.count_bits) h.overflow_l = d.overflow_l;
        }
        if (d.k != a.k || (d.canonical != 0) != a.canonical || (d.acgt_only != 0) != a.acgt_only || d.min_qual_char != a.min_qual_char)
            return refuse(o + paths[i] + " was counted with " + counting_mode_words(d.k, d.canonical != 0, d.acgt_only != 0, d.min_qual_char) +
                          (with ? "; the first table has " + counting_mode_words(a.k, a.canonical, a.acgt_only, a.min_qual_char) +
                                      ": both tables of a set operation need the same"
                                : std::string("; give the same k, --canonical, --acgt-only and --min-qual-char to load it")), 2);
    }
    return pass();
}

static void print_banner(const arguments &a) {
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
}
