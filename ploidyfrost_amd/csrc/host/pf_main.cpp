// `ploidyfrost` -- command line of the MI355X build, same option surface as the reference's
// hot path (reference src/Main.cpp:124-198 getopt string and cases, :278-541 checks, :770-849 dispatch):
//     ploidyfrost -g <BifrostGraph.gfa> -d <KMCDatabase> -o <prefix> [-t T -l L -u U -z Z -M m -D d -G g -v -i]
//     ploidyfrost -g <BifrostGraph.gfa> -f <BifrostGraph.bfg_colors> -d <KMCDatabaseList> [-C <cutoffs>] -o <prefix> ...
// Output: ./PloidyFrost_output/<prefix>_*.txt, byte-identical to the reference run with -t 1.
// The coverage thresholds of the path can be derived from k-mer histograms exactly as in the reference: the
// `cutoffL` / `cutoffU` sub-commands and `-h <histogram>` (with -f: a list of histograms) with `-q <quantile>`
// (src/Main.cpp:200-277, 354-396, 721-762).  `model` (GMM ploidy inference, src/Main.cpp:636-719; the EM on the device) and
// `filter` / `filter-multi` (the row predicates of script/Filter.R, script/Filter-multi.R; host/pf_filter.cpp) are the steps behind
// the path.
#include <sys/prctl.h>
#include <sys/wait.h>
#include <signal.h>
#include <cerrno>
#include <getopt.h>
#include <sys/stat.h>
#include <unistd.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <iostream>
#include <iterator>
#include <sstream>
#include <algorithm>
#include <string>
#include <fstream>
#include <thread>
#include <vector>

#include "pf_cdbg.hpp"
#include "pf_cli_subs.hpp"
#include "pf_cutoffs.hpp"
#include "pf_run_host.hpp"
#include "pf_runmulti_host.hpp"
#include "pf_filter.hpp"
#include "pf_multi.hpp"
#include "pf_gmm_model.hpp"
#include "ploidyfrost_hip.h"

using namespace std;
using namespace pfcli;

namespace {
void PrintUsage() {
    cout << "Usage: PloidyFrost -g <BifrostGraph> -d <KMCDatabase> -o <outfile_prefix> ..." << endl << endl;
    cout << "parameters with required argument:" << endl << endl
         << "  -g,             Input Bifrost Graph file (GFA format)" << endl
         << "  -o,             Prefix for Output files (default : 'output')" << endl
         << "  -t,             Number of Threads (default is 1; output always follows the -t 1 order)" << endl
         << "  -d,             Load KMC Database (with -f: a file listing one database per colour)" << endl
         << "  -f,             Input Bifrost color file (BFG_COLORS format): colored, multi-sample analysis" << endl
         << "  -C,             Coverage thresholds file, one \"lower<TAB>upper\" line per colour (default : 10 1000)" << endl
         << "  -l,             Lower coverage threshold (default : 10 )" << endl
         << "  -u,             Upper coverage threshold (default : 1000 )" << endl
         << "  -z,             Maximum number of unitigs in superbubble (default : 8 )" << endl
         << "  -M,             Match score (default : 2 )" << endl
         << "  -D,             Mismatch penalty (default : -1 )" << endl
         << "  -G,             Gap penalty (default : -3 )" << endl << endl
         << "parameters with no argument:" << endl << endl
         << "  -v,             Print information messages during construction" << endl
         << "  -i,             Output Information about Bifrost graph" << endl << endl
         << "  -h,             k-mer histogram file (with -f: a list of them): thresholds = cutoffL / cutoffU of it" << endl
         << "  -q,             quantile for the upper threshold derived from -h (default : 0.998 )" << endl
         << "  --auto-cutoffs  thresholds = cutoffL / cutoffU (quantile -q) of the k-mer histogram of the database itself (with -f: of every" << endl
         << "                  colour's), counted on the device while it is loaded; instead of -h, -C, -l, -u" << endl
         << "  --ref-threads N N > 1: text format of the reference's `-t N` run (ids from 0, allele_frequency grouped by arity)" << endl
         << "  --gpus N        one graph over N GPUs of this node (single-sample path): one process per GPU, the bubble list cut into N slices," << endl
         << "                  two small all-gathers over RCCL, every rank writes its slabs into the shared result files" << endl
         << "  --detach-teardown  return as soon as the result files are complete; a child process gives the device memory back" << endl
         << "  --model cov|fre    the ploidy estimate in the same run (single-sample path, one GPU): <prefix>_model_result.txt as" << endl
         << "                  `model -f <prefix>` (cov) / `model -g <prefix>_allele_frequency.txt` (fre) writes it, fitted from the" << endl
         << "                  result text while it is on the device; its last line is printed as well" << endl
         << "  --model-ploidy LO:HI  Gaussians to fit, ploidy - 1 (default 1:9; `model -l / -u`)" << endl
         << "  --model-q Q     minimum allele frequency (default 0; `model -q`)" << endl
         << "  --model-m M, --model-n N, --model-iter K, --model-delta A   `model -m / -n / -k / -a` (defaults 5, 2, 1000, 0.01)" << endl
         << "  --model-only    write <prefix>_model_result.txt but none of the ten calling files; their text never leaves the device" << endl
         << "  --filter \"OPTS\"  with --model: the rows through `ploidyfrost filter OPTS` (-S -l -u -I -P -n -d -s -q) first, on the device" << endl
         << "  --filter-multi \"OPTS\"  with -f and --model: the colored rows through `ploidyfrost filter-multi OPTS` (-S -l -u -I -P -n -d -s -q" << endl
         << "                  -c -v) first, on the device; the estimate of that filter and `model` in one command, no filtered table written" << endl
         << "  --model-each-color  with --filter-multi (without -c): one estimate per colour, <prefix>_color<c>_model_result.txt each, as" << endl
         << "                  --filter-multi \"OPTS -c c\" gives them one run at a time" << endl
         << "  --density       with --model: the Gaussian kernel density of the values the model read (the curve of script/Drawfreq.R, as" << endl
         << "                  numbers), <prefix>_allele_frequency_density.txt; with --model-each-color one file per fitted colour" << endl
         << "  --density-points N, --density-adjust A   grid points (default 512, 2 to 4096) and bandwidth factor (default 1)" << endl << endl
         << "Usage: PloidyFrost cutoffL kmer_histogram_file" << endl
         << "Usage: PloidyFrost cutoffU kmer_histogram_file (quantile[<1 ,default:0.998])" << endl
         << "Usage: PloidyFrost cutoffL -d <KMCDatabase>" << endl
         << "Usage: PloidyFrost cutoffU -d <KMCDatabase> (quantile[<1 ,default:0.998])" << endl
         << "Usage: PloidyFrost histogram -d <KMCDatabase> [-o <file>]   (the k-mer histogram file of the database, count<TAB>number per row)" << endl << endl
         << "Usage: PloidyFrost count -k 25 -ci 1 -cs 10000 [-cx N] [-b] -i <reads.fq> [-i <more.fq> ...] -o <KMCDatabase> [--hist <file>] [--chunk-bytes N] [--initial-slots N] [--gz] [--gz-plain] [--fasta] [-v]" << endl
         << "Usage: PloidyFrost mask -d <KMCDatabase> -i <reads.fq> [-i <more.fq> ...] -o <out.fq> (-l L | --auto-cutoffs) [-u U] [--chunk-bytes N] [--gz-out] [-v]" << endl
         << "Usage: PloidyFrost mask -k 25 [-ci N -cs N -cx N -b] -i <reads.fq> ... -o <out.fq> (-l L | --auto-cutoffs) [-u U] [--db-out <KMCDatabase>] [--chunk-bytes N] [--gz-out]" << endl
         << "                  (`kmc_tools filter -hm <db> <reads.fq> -ci<L> [-cx<U>] <out.fq>` on the device: every base of every k-mer whose count" << endl
         << "                  lies outside [L, U] becomes N; --auto-cutoffs: L = what `cutoffL -d` prints, printed on stdout)" << endl << endl
         << "Usage: PloidyFrost trim -i <reads.fq> [-i <more.fq> ...] -o <trimmed.fq> STEP... [--phred 33|64] [--trimlog <file>] [--chunk-bytes N] [--gz] [--gz-plain] [--gz-out] [-v]" << endl
         << "Usage: PloidyFrost trim -1 <r1.fq> -2 <r2.fq> -o1 <p1.fq> -u1 <u1.fq> -o2 <p2.fq> -u2 <u2.fq> STEP... [the same options]" << endl
         << "                  (`trimmomatic SE|PE` on the device; STEP: LEADING:t TRAILING:t SLIDINGWINDOW:w:t MINLEN:l, applied in the order given)" << endl
         << "                  [--adapters <adapters.fa> [--adapter-seed 0..8] [--adapter-score 1..1000]] on trim, run STEP... and run-multi STEP...: adapter read-through is" << endl
         << "                  clipped on the device before the steps (ILLUMINACLIP's simple mode; no STEP is needed beside --adapters, also with -1 / -2)" << endl
         << "                  [--adapter-pairs [--adapter-pair-score 1..1000] [--adapter-pair-min 1..16] [--adapter-keep-both]] with -1 / -2: ILLUMINACLIP's palindrome mode" << endl
         << "                  from the Prefix<X>/1 and Prefix<X>/2 entries of the adapter file; the reverse read of a clipped pair is dropped unless --adapter-keep-both" << endl
         << "                  [--report <report.tsv>] on trim and on run STEP... / run --adapters: the read quality report of the reads as they come and as they are kept" << endl
         << "Usage: PloidyFrost qc (-i <a.fq> [-i <b.fq> ...] | -1 <r1.fq> [-1 ...] -2 <r2.fq> [-2 ...]) -o <report.tsv> [--phred 33|64] [--gz | --gz-plain] [--chunk-bytes N] [-v]" << endl
         << "                  (quality and base content by cycle, read lengths, quality and GC histograms and a hint about the quality offset, accumulated on" << endl
         << "                  the device; one tab-separated text file)" << endl
         << "Usage: PloidyFrost smudge -d <KMCDatabase> (-l L -u U | --auto-cutoffs [-q Q]) -o <out> [-n N] [--pairs <file>] [-v]" << endl
         << "Usage: PloidyFrost smudge -k 25 [-ci 1 -cs 10000 -cx N] -i <reads.fq> [-i <more.fq> ...] (-l L -u U | --auto-cutoffs [-q Q]) -o <out> [-n N] [--pairs <file>]" << endl
         << "                  (a Smudgeplot-style check of the estimate: the pairs of k-mers one substitution apart with no other such neighbour, both" << endl
         << "                  with a count in [L, U], and the table of their two coverages, on the device; <out>_smudge.tsv; -n N: the haploid coverage," << endl
         << "                  for the summary by AB, AAB, AABB ...; run --smudge [--smudge-n N] [--smudge-pairs <file>] writes it beside the estimate)" << endl << endl
         << "Usage: PloidyFrost build -k 25 [-i] [-d] -r <reads.fq> [-r <more.fq> ...] -o <sample> [-g G] [-t N] [--chunk-bytes N] [--initial-slots N] [-v]" << endl
         << "                  (`Bifrost build -r` on the device: <sample>.gfa, the compacted de Bruijn graph of the reads; -i clips tips, -d deletes" << endl
         << "                  isolated unitigs, both of fewer than k k-mers; single-sample graphs from FASTQ only)" << endl
         << "Usage: PloidyFrost build-multi -k 25 [-i] [-d] -r <s0.fq> -r <s1.fq> [-r ...] -o <sample> [-g G] [-t N] [--chunk-bytes N] [--initial-slots N] [-v]" << endl
         << "                  (`Bifrost build -c -r ... -r ...` on the device: <sample>.gfa of all files together, every S line with its DA tag, and" << endl
         << "                  <sample>.bfg_colors, one colour per -r in the order given; what the calling run takes with -g and -f)" << endl << endl
         << "Usage: PloidyFrost run [-k 25 -ci 1 -cs 10000 -cx N] -i <trimmed.fq> [-i <more.fq> ...] -o <sample> [-q Q] [-u U] [--keep-tips] [--keep-isolated] [-g G]" << endl
         << "                  [-z -M -D -G -t --ref-threads] [--model cov|fre ... --model-only --filter \"OPTS\" --density ...] [--db-out <KMCDatabase>] [--gfa-out <sample>]" << endl
         << "                  [--chunk-bytes N] [--initial-slots N] [--gz] [--gz-plain] [--fasta] [-v]" << endl
         << "                  (reads to ploidy estimate in one process: `mask -k ... --auto-cutoffs`, `build -i -d` and the calling run with --auto-cutoffs on" << endl
         << "                  one device context, no masked reads, database or graph file in between; L is printed on stdout)" << endl
         << "Usage: PloidyFrost run [the same options] (-i <raw.fq> [-i <more.fq> ...] | -1 <r1.fq> -2 <r2.fq> [-1 <r3.fq> -2 <r4.fq> ...]) -o <sample> STEP... [--phred 33|64]" << endl
         << "                  (raw reads to ploidy estimate: the reads are trimmed on the device on the way in, as `trim STEP...` trims them; of a pair the" << endl
         << "                  records go on when both are kept; `run-multi` takes STEP... and -1 / -2 inside a --sample likewise)" << endl << endl
         << "Usage: PloidyFrost run-multi [-k 25 -ci 1 -cs 10000 -cx N] --sample <NAME> -i <a.fq> [-i <b.fq> ...] --sample <NAME2> -i <c.fq> [...] -o <out> [-q Q] [-u U]" << endl
         << "                  [--keep-tips] [--keep-isolated] [-g G] [-z -M -D -G -t --ref-threads] [--model cov|fre --filter-multi \"OPTS\" [--model-each-color] [--density ...] [--model-only]]" << endl
         << "                  [--db-out <KMCDatabase>] [--gfa-out <graph>] [--chunk-bytes N] [--initial-slots N] [--gz] [--gz-plain] [--fasta] [-v]" << endl
         << "                  (reads of several samples to one estimate per sample in one process: `mask -k ... --auto-cutoffs` per sample, `build-multi -i -d`" << endl
         << "                  and the coloured calling run with --auto-cutoffs on one device context; a sample is a colour, in the order given; every L on stdout)" << endl << endl
         << "                  (--gz of count, trim, run and run-multi: an input that starts with the gzip magic is blocked gzip -- what bgzip, bcl2fastq2 and" << endl
         << "                  BCL Convert write -- and is inflated on the device; plain gzip is refused: recompress it with bgzip, or decompress it)" << endl
         << "                  (--gz-plain of the same commands implies --gz and takes any other gzip file as well -- what gzip and pigz write, one member or" << endl
         << "                  several -- its deflate streams cut into pieces at block starts and inflated on the device; every member's CRC-32 is checked)" << endl
         << "                  (--fasta of count, build, build-multi, run -i and run-multi -i: an input whose first byte -- with --gz / --gz-plain: first inflated" << endl
         << "                  byte -- is '>' is FASTA, multi-line or not; its records are counted as the same reads in FASTQ would be; FASTA and FASTQ files may be mixed)" << endl << endl
         << "Usage: PloidyFrost model ...          (GMM ploidy inference from the coverage / frequency files; `PloidyFrost model` prints its options)" << endl
         << "Usage: PloidyFrost density -f <column file> -o <outfile_prefix> [-n points] [-a adjust]   (kernel density of a column of numbers)" << endl
         << "Usage: PloidyFrost filter ...         (the row predicates of script/Filter.R over <prefix>_*cov.txt; -h prints its options)" << endl
         << "Usage: PloidyFrost filter-multi ...   (script/Filter-multi.R: the colored tables, with -c colour and -v Cramer's V)" << endl;
}

// the second column of a histogram file, in file order (the parsing of src/Main.cpp:202-225, 238-261)
vector<uint64_t> histogram_rows(const string &file) {
    ifstream f(file);
    if (!f.is_open()) { cout << "ERROR:Open Histogram File " << file << " error!" << endl; exit(EXIT_FAILURE); }
    vector<uint64_t> v;
    string s;
    while (getline(f, s, '\n')) {
        const size_t pos1 = s.find("\t");
        if (pos1 == string::npos) { cerr << "Error: Histogram File is badly Formatted." << endl; exit(EXIT_FAILURE); }
        v.emplace_back((uint64_t)(size_t)atoll(s.substr(pos1 + 1).c_str()));
    }
    return v;
}

// lower threshold: 1.25 x the position of the first local minimum of the histogram (src/Main.cpp:200-235)
int cutoffL(const vector<uint64_t> &rows) {
    int lower = 0, upper = 0;
    (void)pfh::cutoffs_from_rows(rows, 0.998, lower, upper);
    return lower;
}
int cutoffL(const string &file) { return cutoffL(histogram_rows(file)); }

// upper threshold: the multiplicity below which `frequency` of the k-mers beyond the first bin lie (src/Main.cpp:236-277)
int cutoffH(const vector<uint64_t> &rows, double frequency = 0.998) {
    int lower = 0, upper = 0;
    if (pfh::cutoffs_from_rows(rows, frequency, lower, upper)) { cerr << "Error: Histogram File is badly Formatted." << endl; exit(EXIT_FAILURE); }
    return upper;
}
int cutoffH(const string &file, double frequency = 0.998) { return cutoffH(histogram_rows(file), frequency); }

// the rows of a database's k-mer histogram, counted on the device (K-HIST); leaves with the reason when that fails
vector<uint64_t> database_rows(const string &db, uint64_t *min_count = nullptr) {
    vector<uint64_t> rows;
    uint64_t mn = 0;
    string err;
    if (pfh::kmc_histogram(db, 0, rows, mn, err)) { cout << "ERROR: " << err << endl; exit(EXIT_FAILURE); }
    if (min_count) *min_count = mn;
    return rows;
}

bool file_exists(const string &p) {
    struct stat sb;
    return stat(p.c_str(), &sb) == 0;
}

// --filter "<opts>": the words through the option table of `ploidyfrost filter`; what has no meaning in front of the model of the
// same run is refused by name.  false: refused, one line on stderr.
bool parse_filter_words(const string &words, pf_filter_opts &out) {
    std::istringstream in(words);
    vector<string> args;
    for (string w; in >> w;) args.push_back(w);
    pfh::FilterOptions o;
    string err, seen;
    const int ps = pfh::parse_filter_options(args, false, o, err, &seen);
    if (ps == 2) { cerr << "Error: --filter takes the options of `ploidyfrost filter` (-S -l -u -I -P -n -d -s -q), not -h" << endl; return false; }
    if (ps) {
        if (err.rfind("Error: unknown option -c", 0) == 0 || err.rfind("Error: unknown option -v", 0) == 0 || err.rfind("Error: unknown option --color", 0) == 0 ||
            err.rfind("Error: unknown option --cramer", 0) == 0)
            err += " in --filter (filter-multi's option: the colored path has no model in the same run)";
        else err += " in --filter";
        cerr << err << endl;
        return false;
    }
    for (char c : seen)
        if (c == 'i' || c == 'o') {
            cerr << "Error: --filter: -" << c << " has no meaning here (the filter reads this run's own streams and writes no table)" << endl;
            return false;
        }
    if (o.frequency > 0.5) { cerr << "Error: --filter: -q " << o.frequency << ": frequency should < 0.5" << endl; return false; }
    out.simple = o.simple; out.indel = o.indel; out.snp = o.snp;
    out.low = o.low; out.up = o.up; out.num = o.num; out.distance = o.distance; out.size = o.size;
    out.frequency = o.frequency;
    return true;
}

// --filter-multi "<opts>": the same through the option table of `ploidyfrost filter-multi`
bool parse_filter_multi_words(const string &words, pf_filter_multi_opts &out) {
    std::istringstream in(words);
    vector<string> args;
    for (string w; in >> w;) args.push_back(w);
    pfh::FilterOptions o;
    o.multi = true;
    string err, seen;
    const int ps = pfh::parse_filter_options(args, true, o, err, &seen);
    if (ps == 2) { cerr << "Error: --filter-multi takes the options of `ploidyfrost filter-multi` (-S -l -u -I -P -n -d -s -q -c -v), not -h" << endl; return false; }
    if (ps) { cerr << err << " in --filter-multi" << endl; return false; }
    for (char c : seen)
        if (c == 'i' || c == 'o') {
            cerr << "Error: --filter-multi: -" << c << " has no meaning here (the filter reads this run's own streams and writes no table)" << endl;
            return false;
        }
    if (o.frequency > 0.5) { cerr << "Error: --filter-multi: -q " << o.frequency << ": frequency should < 0.5" << endl; return false; }
    out.simple = o.simple; out.indel = o.indel; out.snp = o.snp;
    out.low = o.low; out.up = o.up; out.num = o.num; out.distance = o.distance; out.size = o.size;
    out.frequency = o.frequency;
    out.color = o.color;
    out.cramer = o.cramer;
    return true;
}
bool refuse_each_color_with_one(const pf_filter_multi_opts &m) {
    if (m.color < 0) return false;
    cerr << "Error: --model-each-color fits every colour: --filter-multi holds -c " << m.color << " (one colour: leave --model-each-color out)" << endl;
    return true;
}

// the density of the values `model` has on the device, written beside its result: 0 = ok, 2 = fewer than two values
int density_of(pfh::GmmModel &model, const DensityCli &dc, const string &outprefix, string &err) {
    if (model.size() < 2) { err = "need at least 2 data points"; return 2; }
    pfh::Density d;
    if (model.density(dc.points, dc.adjust, d)) { err = model.error(); return 1; }
    return pfh::write_density(outprefix, d, err);
}

void PrintDensityUsage() {
    cout << "Usage: PloidyFrost density" << endl
         << "Gaussian kernel density of a column of numbers (the curve script/Drawfreq.R draws; the exact sum, on the device)" << endl
         << "  -f,             Column file: one number a line, blank lines and lines beginning with # skipped" << endl
         << "  -o,             Output prefix: <prefix>_allele_frequency_density.txt (default : 'output')" << endl
         << "  -n,             Grid points (default : 512, 2 to 4096)" << endl
         << "  -a,             Bandwidth factor, ggplot2's adjust (default : 1)" << endl
         << endl;
}

// `ploidyfrost density`: Drawfreq.R's numbers (its -t and -p draw and are not taken)
int density_main(int argc, char **argv) {
    string file, outprefix = "output";
    DensityCli dc;
    dc.on = true;
    int oc;
    while ((oc = getopt(argc, argv, "f:o:n:a:")) != -1) {
        switch (oc) {
            case 'f': file = optarg; break;
            case 'o': outprefix = optarg; break;
            case 'n': dc.points_seen = true; dc.points_word = optarg; break;
            case 'a': dc.adjust_seen = true; dc.adjust_word = optarg; break;
            default: PrintDensityUsage(); return 1;
        }
    }
    if (file.empty()) { PrintDensityUsage(); return argc > 2 ? 1 : 0; }
    if (!dc.check("-n", "-a")) return 1;
    if (!file_exists(file)) { cerr << "ERROR: open column file " << file << " error!" << endl; return 1; }
    pfh::GmmModel model;
    string err;
    if (model.readColumn(file)) { cerr << model.error() << endl; return 1; }
    if (density_of(model, dc, outprefix, err)) { cerr << err << endl; return 1; }
    return 0;
}

void PrintModelUsage() {  // src/Main.cpp:694-718
    cout << "Usage: PloidyFrost model" << endl
         << "GMM model" << endl
         << "  -f,             Prefix of coverage files" << endl
         << "  -g,             Allele frequency file" << endl
         << "  -l,             Minimum ploidy level" << endl
         << "  -u,             Maximum ploidy level" << endl
         << "  -q,             Minimum allele frequency" << endl
         << "  -m,             Weigth minimum threshold ( each_weight > 1/(p-1)/m , default value of m is 5)" << endl
         << "  -n,             Weigth minimum threshold ( first_weight > maximum_weight/(p-1)/n , default value of n is 2)" << endl
         << "  -k,             Maximum iterations" << endl
         << "  -a,             Maximum delta" << endl
         << "  -o,             Output prefix" << endl
         << "  --filter \"OPTS\" with -f: the rows of the (unfiltered) coverage files through `ploidyfrost filter OPTS` first, on the device;" << endl
         << "                  add --source fre for the filtered frequencies (as `model -g <filtered>_allele_frequency.txt`)" << endl
         << "  --filter-multi \"OPTS\" with -f: the same for the coverage files of a colored run through `ploidyfrost filter-multi OPTS`;" << endl
         << "                  --model-each-color: one result per colour, <out>_color<c>_model_result.txt" << endl
         << "  --density       the Gaussian kernel density of the values the model read, <out>_allele_frequency_density.txt (per colour:" << endl
         << "                  <out>_color<c>_allele_frequency_density.txt); --density-points N (default 512), --density-adjust A (default 1)" << endl
         << endl;
}

// `PloidyFrost model` (src/Main.cpp:636-719): option defaults, check_Model_ProgramOptions (:542-617), the fits on the device
int model_main(int argc, char **argv) {
    string graphfile, colorfile, outprefix = "output";
    int lower = 1, upper = 9, iters = 1000;
    double frequency = 0, delta = 0.01, mthreshold = 5.0, nthreshold = 2.0;
    // --filter "<opts>" [--source cov|fre] (this build's own switches, taken out of argv before getopt sees them)
    bool filtered = false, multi = false, each_color = false;
    string filter_words, filter_source = "cov";
    DensityCli dc;
    for (int i = 2; i < argc; ++i) {
        if (const int took = dc.take(argc, argv, i)) {
            for (int j = i; j + took <= argc; ++j) argv[j] = j + took < argc ? argv[j + took] : nullptr;
            argc -= took;
            --i;
            continue;
        }
        const bool is_filter = strcmp(argv[i], "--filter") == 0, is_multi = strcmp(argv[i], "--filter-multi") == 0;
        if (strcmp(argv[i], "--model-each-color") == 0) {
            each_color = true;
            for (int j = i; j + 1 <= argc; ++j) argv[j] = j + 1 < argc ? argv[j + 1] : nullptr;
            argc -= 1;
            --i;
        } else
        if ((is_filter || is_multi || strcmp(argv[i], "--source") == 0) && i + 1 < argc) {
            if (is_filter || is_multi) {
                if (filtered) { cerr << "Error: --filter and --filter-multi do not go together (one table layout a run)" << endl; return 1; }
                filtered = true; multi = is_multi; filter_words = argv[i + 1];
            }
            else filter_source = argv[i + 1];
            for (int j = i; j + 2 <= argc; ++j) argv[j] = j + 2 < argc ? argv[j + 2] : nullptr;
            argc -= 2;
            --i;
        }
    }
    pf_filter_opts fopts = {};
    pf_filter_multi_opts mopts = {};
    if (each_color && !multi) { cerr << "Error: --model-each-color needs --filter-multi \"OPTS\" (the colour is a column of the colored tables)" << endl; return 1; }
    if (filtered && !(multi ? parse_filter_multi_words(filter_words, mopts) : parse_filter_words(filter_words, fopts))) return 1;
    if (each_color && refuse_each_color_with_one(mopts)) return 1;
    if (filtered && filter_source != "cov" && filter_source != "fre") { cerr << "Error: --source " << filter_source << ": cov or fre" << endl; return 1; }
    if (!dc.check()) return 1;
    int oc;
    while ((oc = getopt(argc, argv, "M:D:G:z:a:l:q:u:e:C:R:o:t:g:f:k:d:m:n:h:ibvpNSc")) != -1) {
        switch (oc) {
            case 'q': frequency = atof(optarg); break;
            case 'm': mthreshold = atof(optarg); break;
            case 'n': nthreshold = atof(optarg); break;
            case 'l': lower = atoi(optarg); break;
            case 'u': upper = atoi(optarg); break;
            case 'a': delta = atof(optarg); break;
            case 'o': outprefix = optarg; break;
            case 'g': graphfile = optarg; break;
            case 'f': colorfile = optarg; break;
            case 'k': iters = atoi(optarg); break;
            default: break;
        }
    }
    bool ok = true;
    if (lower > upper) { cerr << "Error:  min gauss <= max gauss  " << endl; ok = false; }
    if (lower < 1 || upper < 1) { cerr << "Error: gauss > 0  " << endl; ok = false; }
    if (frequency >= 0.5) { cerr << "Error: frequency cutoff value should < 0.5  " << endl; ok = false; }
    if (iters < 0) { cerr << "Error: iterate count should > 0 " << endl; ok = false; }
    if (delta < 0) { cerr << "Error: iterate delta should > 0 " << endl; ok = false; }
    if (mthreshold < 0) { cerr << "Error: minimum threshold should > 0 " << endl; ok = false; }
    if (nthreshold < 0) { cerr << "Error: minimum threshold should > 0 " << endl; ok = false; }
    if (colorfile.empty() && graphfile.empty()) { cout << "ERROR: input a frequency or coverage file " << endl; ok = false; }
    if (!graphfile.empty() && !file_exists(graphfile)) { cout << "ERROR: open frequency file " << graphfile << " error!" << endl; ok = false; }
    if (filtered && colorfile.empty()) { cerr << "Error: model --filter reads the coverage files of a prefix: give it with -f" << endl; return 1; }
    if (filtered && !file_exists(colorfile + "_pentacov.txt")) { cout << "ERROR: open coverage file " << colorfile + "_pentacov.txt" << " error!" << endl; ok = false; }
    if (!colorfile.empty())
        for (const char *suf : {"_bicov.txt", "_tricov.txt", "_tetracov.txt"})
            if (!file_exists(colorfile + suf)) { cout << "ERROR: open coverage file " << colorfile + suf << " error!" << endl; ok = false; }
    if (ok && upper > PF_GMM_MAX_GAUSS) { cerr << "Error: this build fits at most " << PF_GMM_MAX_GAUSS << " Gaussians (-u)" << endl; ok = false; }
    if (!ok) { PrintModelUsage(); return 0; }
    pfh::GmmModel model;
    model.setMThreshold(mthreshold);
    model.setNThreshold(nthreshold);
    model.setMaxIterNum(iters);
    model.setMaxDeltaNum(delta);
    if (filtered) {
        // the filter and the fit in one command from files: the four tables through the kernels of the one-command run
        // (pf_call_model_take_text), pieces of at most 1 MB cut behind line feeds
        pf_ctx *ctx = nullptr;
        auto leave = [&](const string &m) {
            cout << m << endl;
            exit(EXIT_FAILURE);
        };
        if (pf_create(0, &ctx) != PF_OK) leave(string("GmmModel: no device context (") + (pf_last_error(nullptr) ? pf_last_error(nullptr) : "?") + "); the fit runs on the GPU only");
        if (pf_call_model_begin(ctx, filter_source == "cov" ? PF_MODEL_COV : PF_MODEL_FRE, frequency) != PF_OK || (multi ? pf_call_model_filter_multi(ctx, &mopts, each_color ? 1 : 0) : pf_call_model_filter(ctx, &fopts)) != PF_OK) leave(pf_last_error(ctx));
        int ord = 0;
        for (const char *suf : {"_bicov.txt", "_tricov.txt", "_tetracov.txt", "_pentacov.txt"}) {
            ifstream in(colorfile + suf, std::ios::binary);
            const string text((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
            for (size_t at = 0; at < text.size();) {
                size_t end = std::min(text.size(), at + ((size_t)1 << 20));
                if (end < text.size()) {
                    const size_t nl = text.rfind('\n', end - 1);
                    if (nl != string::npos && nl >= at) end = nl + 1;
                    else { const size_t next = text.find('\n', end); end = next == string::npos ? text.size() : next + 1; }
                }
                if (pf_call_model_take_text(ctx, ord, text.data() + at, end - at) != PF_OK) leave(pf_last_error(ctx));
                at = end;
            }
            ++ord;
        }
        uint64_t n_values = 0;
        if (pf_call_model_finish(ctx, &n_values) != PF_OK) leave(pf_last_error(ctx));
        if (each_color) {   // one result per colour that kept a row, in colour order
            // (colours above the largest one that kept a row are not known here -- the tables do not say how many there are -- so
            // they get no line; the run with -f <colors file> names every colour of the graph)
            const uint32_t nc = pf_call_model_color_count(ctx);
            uint32_t fitted = 0, curves = 0;
            for (uint32_t c = 0; c < nc; ++c) {
                uint64_t n_c = 0;
                if (pf_call_model_color_select(ctx, (int)c, &n_c) != PF_OK) leave(pf_last_error(ctx));
                if (n_c == PF_MODEL_NO_ROW) { cerr << "color " << c << ": no row kept, no estimate" << endl; continue; }
                if (n_c == 0) { cerr << "color " << c << ": the rows kept hold no value for the model, no estimate" << endl; continue; }
                pfh::GmmModel cm;
                cm.setMThreshold(mthreshold);
                cm.setNThreshold(nthreshold);
                cm.setMaxIterNum(iters);
                cm.setMaxDeltaNum(delta);
                cm.borrow(ctx, (size_t)n_c);
                string cerr_;
                double ploidy = 0;
                if (pfh::run_model(cm, lower, upper, outprefix + "_color" + to_string(c), cerr_, &ploidy)) leave(cerr_);
                cout << "color " << c << ": estimated ploidy level is : " << ploidy << endl;
                ++fitted;
                if (dc.on) {
                    const int ds = density_of(cm, dc, outprefix + "_color" + to_string(c), cerr_);
                    if (ds == 1) leave(cerr_);
                    if (ds == 2) cerr << "color " << c << ": " << cerr_ << ", no density" << endl;
                    else ++curves;
                }
            }
            pf_destroy(ctx);
            if (!fitted) { cout << "model --model-each-color: no colour holds a value for the model" << endl; return EXIT_FAILURE; }
            if (dc.on && !curves) { cout << "need at least 2 data points" << endl; return EXIT_FAILURE; }
            return 0;
        }
        model.borrow(ctx, (size_t)n_values);
    } else
    if (!colorfile.empty() ? model.readCovFile(colorfile, frequency) : model.readFreFile(graphfile, frequency)) {
        cout << model.error() << endl;
        exit(EXIT_FAILURE);
    }
    string err;
    if (pfh::run_model(model, lower, upper, outprefix, err)) {
        cout << err << endl;
        exit(EXIT_FAILURE);
    }
    if (dc.on && density_of(model, dc, outprefix, err)) {
        cout << err << endl;
        exit(EXIT_FAILURE);
    }
    return 0;
}
}  // namespace

int calling_main(Options &opt, DensityCli &dc);

// (the reads sub-commands -- count, mask, smudge, qc, trim, build, build-multi, run, run-multi -- have their command lines in
// pf_cli_reads.cpp, pf_cli_build.cpp and pf_cli_run.cpp; pf_cli_subs.hpp declares them)
int main(int argc, char **argv) {
    if (argc < 2) { PrintUsage(); return 0; }
    if (!strcmp(argv[1], "run-multi")) return run_multi_main(argc, argv);
    if (!strcmp(argv[1], "run")) return run_main(argc, argv);
    if (!strcmp(argv[1], "model")) return model_main(argc, argv);
    if (!strcmp(argv[1], "density")) return density_main(argc - 1, argv + 1);
    if (!strcmp(argv[1], "filter")) return pfh::filter_main(argc, argv, false);         // script/Filter.R
    if (!strcmp(argv[1], "filter-multi")) return pfh::filter_main(argc, argv, true);    // script/Filter-multi.R
    if (!strcmp(argv[1], "mask")) return mask_main(argc, argv);
    if (!strcmp(argv[1], "count")) return count_main(argc, argv);
    if (!strcmp(argv[1], "build")) return build_main(argc, argv, false);
    if (!strcmp(argv[1], "build-multi")) return build_main(argc, argv, true);
    if (!strcmp(argv[1], "trim")) return trim_main(argc, argv);
    if (!strcmp(argv[1], "qc")) return qc_main(argc, argv);
    if (!strcmp(argv[1], "smudge")) return smudge_main(argc, argv);
    if (!strcmp(argv[1], "histogram")) {   // the file `kmc_tools transform <db> histogram <file>` writes, from the database on the device
        string db, out;
        for (int i = 2; i < argc; ++i) {
            if (!strcmp(argv[i], "-d") && i + 1 < argc) db = argv[++i];
            else if (!strcmp(argv[i], "-o") && i + 1 < argc) out = argv[++i];
            else { db.clear(); break; }
        }
        if (db.empty()) { cout << "Usage:PloidyFrost histogram -d kmc_database [-o kmer_histogram_file]" << endl; exit(EXIT_FAILURE); }
        uint64_t min_count = 0;
        const vector<uint64_t> rows = database_rows(db, &min_count);
        const string text = pfh::histogram_text(min_count, rows);
        if (out.empty()) { cout << text; return 0; }
        ofstream f(out, std::ios::binary);
        if (!f.is_open() || !(f << text) || !f.flush()) { cout << "ERROR:Write Histogram File " << out << " error!" << endl; exit(EXIT_FAILURE); }
        return 0;
    }
    if (!strcmp(argv[1], "cutoffL") && argc == 4 && !strcmp(argv[2], "-d")) {   // the same from the database itself
        cout << max(10, cutoffL(database_rows(argv[3]))) << endl;
        return 0;
    }
    if (!strcmp(argv[1], "cutoffU") && (argc == 4 || argc == 5) && !strcmp(argv[2], "-d")) {
        const char *usage = "Usage:PloidyFrost cutoffU -d kmc_database (quantile[<1 ,default:0.998]) ";
        if (argc == 4) {
            cout << cutoffH(database_rows(argv[3])) << endl;
        } else {
            double y;
            try { y = stod(argv[4]); } catch (const exception &) { cout << usage << endl; exit(EXIT_FAILURE); }
            if (y >= 1) { cout << usage << endl; exit(EXIT_FAILURE); }
            cout << cutoffH(database_rows(argv[3]), y);
        }
        return 0;
    }
    if (!strcmp(argv[1], "cutoffL")) {  // src/Main.cpp:721-730
        if (argc != 3) { cout << "Usage:PloidyFrost cutoffL kmer_histogram_file" << endl; exit(EXIT_FAILURE); }
        cout << max(10, cutoffL(argv[2])) << endl;
        return 0;
    }
    if (!strcmp(argv[1], "cutoffU")) {  // src/Main.cpp:731-762 (no newline after the value when a quantile is given)
        const char *usage = "Usage:PloidyFrost cutoffU kmer_histogram_file (quantile[<1 ,default:0.998]) ";
        if (argc == 3) {
            cout << cutoffH(argv[2]) << endl;
        } else if (argc == 4) {
            double y;
            try { y = stod(argv[3]); } catch (const exception &) { cout << usage << endl; exit(EXIT_FAILURE); }
            if (y >= 1) { cout << usage << endl; exit(EXIT_FAILURE); }
            cout << cutoffH(argv[2], y);
        } else {
            cout << usage << endl;
            exit(EXIT_FAILURE);
        }
        return 0;
    }
    Options opt;
    DensityCli dc;
    if (!take_long_options(argc, argv, 1, opt, dc)) return 1;
    int oc;
    while ((oc = getopt(argc, argv, "M:D:G:z:a:l:q:u:e:C:R:o:t:g:f:k:d:m:n:h:ibvpNSc")) != -1) {
        switch (oc) {
            case 'z': opt.complex_size = (size_t)atoi(optarg); break;
            case 'M': opt.match = atof(optarg); break;
            case 'D': opt.mismatch = atof(optarg); break;
            case 'G': opt.gap = atof(optarg); break;
            case 'u': opt.coverage_upper = atoi(optarg); opt.u_seen = true;  // falls through, as in the reference (:149-153)
            case 'C': opt.coveragefile = optarg; if (oc == 'C') opt.cfile_seen = true; break;
            case 'h': opt.hist = optarg; break;
            case 'g': opt.graphfile = optarg; break;
            case 'f': opt.colorfile = optarg; break;
            case 'o': opt.outprefix = optarg; break;
            case 'l': opt.coverage_lower = atoi(optarg); opt.l_seen = true; break;
            case 't': opt.nb_threads = (size_t)atoi(optarg); break;
            case 'k': opt.k = atoi(optarg); break;
            case 'v': opt.verbose = true; break;
            case 'd': opt.db = optarg; break;
            case 'i': opt.info = true; break;
            case 'q': opt.frequency = atof(optarg); break;
            case 'm': case 'n': case 'a': case 'b': case 'p': break;  // accepted, no effect on this path
            default:
                cout << "Invalid option" << endl;
                PrintUsage();
                exit(EXIT_FAILURE);
        }
    }
    return calling_main(opt, dc);
}

// The long options of the calling run, this build's own switches, taken out of argv[first ..] before getopt (or `run`'s own loop) sees
// what is left.  --ref-threads N: write the text format of the reference's `-t N` functions -- with N > 1: ids and var_count from 0,
// allele_frequency rows grouped by arity per bubble -- whatever -t says.  false: refused, one line on stderr.
bool take_long_options(int &argc, char **argv, int first, Options &opt, DensityCli &dc) {
    for (int i = first; i < argc; ++i) {
        if (const int took = dc.take(argc, argv, i)) {
            for (int j = i; j + took <= argc; ++j) argv[j] = j + took < argc ? argv[j + took] : nullptr;
            argc -= took;
            --i;
        } else
        if (strcmp(argv[i], "--ref-threads") == 0 && i + 1 < argc) {
            opt.ref_threads = (size_t)atoi(argv[i + 1]);
            for (int j = i; j + 2 <= argc; ++j) argv[j] = j + 2 < argc ? argv[j + 2] : nullptr;
            argc -= 2;
            --i;
        } else if (strcmp(argv[i], "--gpus") == 0 && i + 1 < argc) {
            opt.gpus = (size_t)std::max(1, atoi(argv[i + 1]));
            opt.gpus_seen = true;
            for (int j = i; j + 2 <= argc; ++j) argv[j] = j + 2 < argc ? argv[j + 2] : nullptr;
            argc -= 2;
            --i;
        } else if (strcmp(argv[i], "--detach-teardown") == 0 || strcmp(argv[i], "--model-only") == 0) {
            if (argv[i][2] == 'd') opt.detach_teardown = true;
            else opt.model_only = opt.model_option_seen = true;
            for (int j = i; j + 1 <= argc; ++j) argv[j] = j + 1 < argc ? argv[j + 1] : nullptr;
            argc -= 1;
            --i;
        } else if (strcmp(argv[i], "--model-each-color") == 0 || strcmp(argv[i], "--auto-cutoffs") == 0) {
            if (argv[i][2] == 'a') opt.auto_cutoffs = true;
            else opt.each_color = true;
            for (int j = i; j + 1 <= argc; ++j) argv[j] = j + 1 < argc ? argv[j + 1] : nullptr;
            argc -= 1;
            --i;
        } else if (strcmp(argv[i], "--filter-multi") == 0 && i + 1 < argc) {
            opt.multi_seen = true;
            opt.multi_words = argv[i + 1];
            for (int j = i; j + 2 <= argc; ++j) argv[j] = j + 2 < argc ? argv[j + 2] : nullptr;
            argc -= 2;
            --i;
        } else if (strcmp(argv[i], "--filter") == 0 && i + 1 < argc) {
            opt.filter_seen = true;
            opt.filter_words = argv[i + 1];
            for (int j = i; j + 2 <= argc; ++j) argv[j] = j + 2 < argc ? argv[j + 2] : nullptr;
            argc -= 2;
            --i;
        } else if (strncmp(argv[i], "--model", 7) == 0 && i + 1 < argc) {
            const string name = argv[i], val = argv[i + 1];
            if (name == "--model") opt.model_source = val;
            else if (name == "--model-ploidy") opt.model_ploidy = val;
            else if (name == "--model-q") opt.model_q = atof(val.c_str());
            else if (name == "--model-m") opt.model_m = atof(val.c_str());
            else if (name == "--model-n") opt.model_n = atof(val.c_str());
            else if (name == "--model-iter") opt.model_iter = atoi(val.c_str());
            else if (name == "--model-delta") opt.model_delta = atof(val.c_str());
            else { cerr << "Error: unknown option " << name << endl; return false; }
            opt.model_option_seen = true;
            for (int j = i; j + 2 <= argc; ++j) argv[j] = j + 2 < argc ? argv[j + 2] : nullptr;
            argc -= 2;
            --i;
        }
    }
    return true;
}

// --model / --filter / --filter-multi / --density: refused here, before anything is read or written; the settings of the run
bool model_setup(const Options &opt, DensityCli &dc, pfh::CDBG::ModelOptions &model, pf_filter_opts &filter, pf_filter_multi_opts &multi) {
    if (opt.filter_seen) {
        if (opt.model_source.empty()) { cerr << "Error: --filter stands in front of the model of the same run: it needs --model cov|fre (the filtered tables themselves: `ploidyfrost filter`)" << endl; return false; }
        if (!opt.colorfile.empty()) { cerr << "Error: --filter reads the single-sample result streams; with -f the coverage tables have other columns (the colored path has --filter-multi)" << endl; return false; }
        if (opt.gpus > 1) { cerr << "Error: --filter and --gpus " << opt.gpus << " do not go together (each rank holds a slice of the rows)" << endl; return false; }
        if (!parse_filter_words(opt.filter_words, filter)) return false;
    }
    if (opt.each_color && !opt.multi_seen) { cerr << "Error: --model-each-color needs --filter-multi \"OPTS\" (the colour is a column of the colored tables)" << endl; return false; }
    if (opt.multi_seen) {
        if (opt.filter_seen) { cerr << "Error: --filter-multi and --filter do not go together (one table layout a run)" << endl; return false; }
        if (opt.model_source.empty()) { cerr << "Error: --filter-multi stands in front of the model of the same run: it needs --model cov|fre (the filtered tables themselves: `ploidyfrost filter-multi`)" << endl; return false; }
        if (opt.gpus > 1) { cerr << "Error: --filter-multi and --gpus " << opt.gpus << " do not go together (the colored path runs on one GPU)" << endl; return false; }
        if (opt.colorfile.empty()) { cerr << "Error: --filter-multi reads the colored result streams: it needs -f (the single-sample path has --filter)" << endl; return false; }
        if (!parse_filter_multi_words(opt.multi_words, multi)) return false;
        if (opt.each_color && refuse_each_color_with_one(multi)) return false;
    }
    if (opt.model_option_seen) {
        if (opt.model_source.empty()) { cerr << "Error: the --model-... options need --model cov|fre" << endl; return false; }
        if (opt.model_source != "cov" && opt.model_source != "fre") { cerr << "Error: --model " << opt.model_source << ": the source is cov or fre" << endl; return false; }
        if (!opt.colorfile.empty() && !opt.multi_seen) {
            cerr << "Error: --model reads the single-sample result streams; with -f the coverage tables have other columns and pool every sample: put --filter-multi \"OPTS\" in front of it" << endl;
            return false;
        }
        if (opt.gpus > 1) { cerr << "Error: --model and --gpus " << opt.gpus << " do not go together (each rank holds a slice of the values)" << endl; return false; }
        int lo = 0, hi = 0;
        char tail = 0;
        if (sscanf(opt.model_ploidy.c_str(), "%d:%d%c", &lo, &hi, &tail) != 2 || lo < 1 || hi < lo || hi > PF_GMM_MAX_GAUSS) {
            cerr << "Error: --model-ploidy " << opt.model_ploidy << ": LO:HI Gaussians with 1 <= LO <= HI <= " << PF_GMM_MAX_GAUSS << endl;
            return false;
        }
        if (opt.model_q >= 0.5) { cerr << "Error: --model-q: frequency cutoff value should < 0.5" << endl; return false; }
        if (opt.model_iter < 0) { cerr << "Error: --model-iter: iterate count should > 0" << endl; return false; }
        if (opt.model_delta < 0) { cerr << "Error: --model-delta: iterate delta should > 0" << endl; return false; }
        if (opt.model_m < 0 || opt.model_n < 0) { cerr << "Error: --model-m / --model-n: minimum threshold should > 0" << endl; return false; }
        model.on = true;
        model.only = opt.model_only;
        model.source = opt.model_source == "cov" ? PF_MODEL_COV : PF_MODEL_FRE;
        model.q = opt.model_q;
        model.lo = lo; model.hi = hi;
        model.m_thre = opt.model_m; model.n_thre = opt.model_n; model.max_iter = opt.model_iter; model.max_delta = opt.model_delta;
    }
    if (!dc.check()) return false;
    if (dc.on && !model.on) { cerr << "Error: --density takes the density of the values the model of the same run reads: it needs --model cov|fre (a column of numbers: `ploidyfrost density`)" << endl; return false; }
    return true;
}

// the calling run: `ploidyfrost -g <graph> -d <database> ...`, single-sample or colored
int calling_main(Options &opt, DensityCli &dc) {
    // --auto-cutoffs: the thresholds come from the database itself; every other source of them is refused by name, before anything
    // is read or written
    if (opt.auto_cutoffs) {
        const char *with = !opt.hist.empty() ? "-h (one source of thresholds a run: the histogram file or the database)"
                         : opt.cfile_seen ? "-C (one source of thresholds a run: the coverage file or the databases)"
                         : opt.l_seen ? "-l (the lower threshold is derived: leave it out)"
                         : opt.u_seen ? "-u (the upper threshold is derived: leave it out)" : nullptr;
        if (with) { cerr << "Error: --auto-cutoffs does not go with " << with << endl; return 1; }
        if (opt.gpus > 1) { cerr << "Error: --auto-cutoffs and --gpus " << opt.gpus << " do not go together (every rank would count the whole database)" << endl; return 1; }
        opt.coveragefile.clear();
    }
    // --model: refused here, before anything is read or written
    pfh::CDBG::ModelOptions model;
    pf_filter_opts filter = {};
    pf_filter_multi_opts multi = {};
    if (!model_setup(opt, dc, model, filter, multi)) return 1;
    // check_ProgramOptions (:278-541), single-sample subset
    bool ok = true;
    const size_t max_threads = std::thread::hardware_concurrency();
    if ((long)opt.nb_threads <= 0) { cerr << "Error: Number of threads cannot be less than or equal to 0." << endl; ok = false; }
    if (opt.nb_threads > max_threads) { cerr << "Error: Number of threads cannot be greater than or equal to " << max_threads << "." << endl; ok = false; }
    if (opt.frequency < 0 || opt.frequency > 1) { cerr << "Error: frequency cutoff value should be between 0 and 1 " << endl; ok = false; }
    size_t kmc_db_num = 0;
    if (opt.db.empty()) { cerr << "Error: Need input a kmc database prefix!\n"; ok = false; }
    else if (opt.colorfile.empty()) {
        if (!file_exists(opt.db + ".kmc_pre") || !file_exists(opt.db + ".kmc_suf")) {
            cerr << "Error: Could not read the input kmc database " << opt.db << "." << endl;
            ok = false;
        }
        if (!opt.hist.empty()) {  // :354-358
            opt.coverage_lower = max(10, cutoffL(opt.hist));
            opt.coverage_upper = cutoffH(opt.hist, opt.frequency);
        }
    } else {
        // :326-353: the -d file lists one database per line
        ifstream in(opt.db);
        if (!file_exists(opt.db) || in.fail()) { ok = false; }
        else {
            string name;
            while (getline(in, name, '\n')) {
                ++kmc_db_num;
                if (!file_exists(name + ".kmc_pre") || !file_exists(name + ".kmc_suf")) {
                    cerr << "Error: Could not read the input kmc database " << name << "." << endl;
                    ok = false;
                    break;
                }
            }
        }
        if (!opt.hist.empty()) {  // :359-396: one histogram file per line, one per database
            ifstream hin(opt.hist);
            if (!file_exists(opt.hist) || hin.fail()) { ok = false; }
            else {
                string name;
                size_t i = 0;
                while (getline(hin, name, '\n')) {
                    opt.coverage_vec.push_back({max(10, cutoffL(name)), cutoffH(name, opt.frequency)});
                    if (opt.coverage_vec[i].first > opt.coverage_vec[i].second) { cerr << "Error: lower cutoff need be smaller than upper cutoff " << endl; ok = false; }
                    i++;
                }
                if (i != kmc_db_num) { cerr << "ERROR: the numbers of kmc databases and hist files are not equal! " << endl; exit(EXIT_FAILURE); }
            }
        } else
        // :398-455: -C "lower\tupper" per database, default (10, 1000)
        if (!opt.coveragefile.empty()) {
            ifstream cin_(opt.coveragefile);
            if (!file_exists(opt.coveragefile) || cin_.fail()) { ok = false; }
            else {
                string line;
                size_t i = 0;
                while (getline(cin_, line, '\n')) {
                    const size_t pos1 = line.find("\t");
                    if (pos1 == string::npos) { cerr << "Error: Coverage File is badly Formatted." << endl; exit(EXIT_FAILURE); }
                    opt.coverage_vec.push_back({(int)atoll(line.substr(0, pos1).c_str()), (int)atoll(line.substr(pos1 + 1).c_str())});
                    if (opt.coverage_vec[i].first < 0 || opt.coverage_vec[i].second < 0) { cerr << "Error: Filter coverage need a positive number." << endl; ok = false; }
                    if (opt.coverage_vec[i].first > opt.coverage_vec[i].second) { cerr << "Error: lower cutoff need be smaller than upper cutoff " << endl; ok = false; }
                    i++;
                }
                if (i != kmc_db_num) { cerr << "ERROR: the numbers of kmc databases and coverages are not equal! " << endl; exit(EXIT_FAILURE); }
            }
        } else {
            opt.coverage_vec.insert(opt.coverage_vec.end(), kmc_db_num, pair<int, int>(10, 1000));
        }
        if (!file_exists(opt.colorfile)) { cerr << "Error: The input color file does not exist." << endl; ok = false; }
    }
    if (opt.complex_size < 4) { cerr << "Error: Maximum number of unitigs in superbubble is at least 4 !" << endl; ok = false; }
    if (opt.mismatch > opt.match) { cerr << "Error: Mismatch penalty should be smaller than match score !" << endl; ok = false; }
    if (opt.gap > opt.match) { cerr << "Error: Gap penalty should be smaller than match score !" << endl; ok = false; }
    if (opt.outprefix.empty()) { cerr << "Error: No output filename prefix given." << endl; ok = false; }
    if (opt.coverage_lower < 0 || opt.coverage_upper < 0) { cerr << "Error: Filter coverage need a positive number." << endl; ok = false; }
    if (opt.coverage_lower > opt.coverage_upper) { cerr << "Error: lower cutoff need be smaller than upper cutoff " << endl; ok = false; }
    if (opt.graphfile.empty()) { cerr << "Error: No graph file was provided in input." << endl; ok = false; }
    else if (!file_exists(opt.graphfile)) { cerr << "Error: The graph file does not exist." << endl; ok = false; }
    if (!ok) { PrintUsage(); return 0; }

    if (!opt.colorfile.empty() && opt.gpus > 1) { cerr << "Error: --gpus cuts the single-sample path (-g / -d); the colored one runs on one GPU" << endl; return 1; }
    if (!opt.colorfile.empty()) {  // src/Main.cpp:775-810
        pfh::ColoredUnitigSet cdbg;
        auto t0 = std::chrono::steady_clock::now();
        if (!cdbg.read(opt.graphfile, opt.colorfile, opt.nb_threads, opt.verbose)) {
            cout << "ColoredCDBG::read(): Graph could not be loaded! Exit. (" << cdbg.err << ")" << endl;
            exit(EXIT_FAILURE);
        }
        cout << "ColoredCDBG::read(): Graph loading successful" << endl;

        cout << "CCDBG: Graph loading Real time : " << std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() << "s" << endl;
        if (cdbg.getNbColors() != kmc_db_num) {
            cerr << "CCDBG::CCDBG():Error: " << kmc_db_num << " kmc databases listed for " << cdbg.getNbColors() << " colors" << endl;
            exit(EXIT_FAILURE);
        }
        vector<vector<uint64_t>> color_rows;
        pfh::CCDBG g(cdbg, opt.complex_size, opt.match, opt.mismatch, opt.gap, opt.db, opt.nb_threads, 0, false, opt.auto_cutoffs ? &color_rows : nullptr);
        if (opt.verbose && cdbg.graph.n_abundant)
            cout << "ColoredCDBG::read(): " << cdbg.graph.n_abundant << " k-length unitigs are abundant k-mers (numbered last, in Bifrost's hash table order)" << endl;
        auto die = [&]() {
            cerr << g.error() << endl;
            exit(EXIT_FAILURE);
        };
        if (!g.good()) die();
        pfh::ColoredCallSetup call;
        call.outprefix = opt.outprefix;
        call.graphfile = opt.graphfile;
        call.threads = opt.nb_threads;
        call.info = opt.info;
        call.verbose = opt.verbose;
        call.model = model;
        call.filter_multi = opt.multi_seen ? &multi : nullptr;
        call.each_color = opt.each_color;
        call.density_points = dc.on ? dc.points : 0;
        call.density_adjust = dc.adjust;
        call.cutoffs = opt.coverage_vec;
        call.color_rows = opt.auto_cutoffs ? &color_rows : nullptr;
        call.quantile = opt.frequency;
        string call_err;
        if (pfh::colored_call_run(g, call, call_err)) {
            cerr << call_err << endl;
            exit(EXIT_FAILURE);
        }
        return 0;
    }

    // Giving 12 GB of device memory and the pinned buffers back is 0.35-0.4 s of driver work at process exit (5 M unitigs) --
    // a third of the whole run.  On request (--detach-teardown) that work is done by a child process:
    // the parent returns the moment the child reports that the last result file is complete, the child finishes its exit with
    // nobody waiting for it -- and still holds its device memory for those 0.4 s, which a scheduler that starts the next job on
    // the parent's return has to know; hence not the default.  (Forked here, before the first thread and the first device call.)
    int done_fd = -1;
    if (opt.detach_teardown) {
        int fds[2];
        if (pipe(fds) == 0) {
            cout.flush();
            fflush(nullptr);
            const pid_t pid = fork();
            if (pid > 0) {
                close(fds[1]);
                unsigned char code = 0;
                ssize_t n;
                do n = read(fds[0], &code, 1); while (n < 0 && errno == EINTR);
                if (n == 1) _exit(code);
                int st = 0;   // the child left without reporting: its exit status is the run's
                while (waitpid(pid, &st, 0) < 0 && errno == EINTR) {}
                _exit(WIFEXITED(st) ? WEXITSTATUS(st) : 128 + (WIFSIGNALED(st) ? WTERMSIG(st) : 0));
            }
            if (pid == 0) {
                close(fds[0]);
                done_fd = fds[1];
                prctl(PR_SET_PDEATHSIG, SIGTERM);   // an interrupted parent takes the run with it
            } else {
                close(fds[0]);
                close(fds[1]);
            }
        }
    }
    // --gpus N: the other ranks are forked here, before anything has touched the GPU (pf_multi.hpp); from here on every rank runs the
    // same program on its own device, rank 0 speaks
    pfh::RankGroup ranks;
    if (opt.gpus > 1) {
        if (opt.ref_threads > 1) { cerr << "Error: --gpus and --ref-threads do not go together" << endl; return 1; }
        cout.flush();
        fflush(nullptr);
        if (!ranks.start((int)opt.gpus)) { cerr << "Error: --gpus " << opt.gpus << ": " << ranks.err << endl; return 1; }
        if (ranks.rank != 0) {   // the other ranks say nothing
            if (!freopen("/dev/null", "w", stdout)) {}
        }
    }
    // the device context and the count table are built on a helper thread while the graph file is read
    pfh::CountsLoader counts;
    counts.want_rows = opt.auto_cutoffs;
    counts.start(ranks.device(), opt.db);
    pfh::UnitigSet graph;
    std::string err;
    auto t0 = std::chrono::steady_clock::now();
    const bool trace_main = getenv("PF_TRACE_LOAD") != nullptr;
    auto mark = [&](const char *what) {
        if (trace_main) fprintf(stderr, "[main] %-28s %.3fs since start\n", what, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    };
    // K-GFA: the file is mapped and its header read here; the segments are parsed and packed on the device by the CDBG constructor
    // (PF_GFA=host: the host loader).  Abundant k-mers are decided there as well (K-MINZ).
    static const bool host_gfa = [] { const char *e = getenv("PF_GFA"); return e && !strcmp(e, "host"); }();
    if (!(host_gfa ? graph.load_gfa(opt.graphfile, err, true) : graph.open_gfa(opt.graphfile, err))) {
        cout << "CompactedDBG::read(): Graph could not be loaded! Exit. (" << err << ")" << endl;
        exit(EXIT_FAILURE);
    }
    if (host_gfa) {
        cout << "CompactedDBG::read(): Graph loading successful" << endl;
        cout << "CDBG: Graph loading Real time : " << std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() << "s" << endl;
    } else if (pf_ctx *c = counts.wait_context()) {
        graph.parse_on_device(c);   // beside the count table's ingest; a refusal is reported by the constructor
    }
    mark("graph file read");

    // (on the heap and never destroyed: at the end of main the process leaves through quick_exit -- giving 12 GB of device and
    // pinned memory back piece by piece takes longer than some of the phases)
    pfh::CDBG &g = *new pfh::CDBG(graph, opt.complex_size, opt.match, opt.mismatch, opt.gap, opt.db, ranks.device(), false, &counts);
    mark("graph + counts on the device");
    auto die = [&]() {
        cerr << g.error() << endl;
        exit(EXIT_FAILURE);
    };
    if (!g.good() && ranks.world <= 1) {
        if (g.error().rfind("CompactedDBG::read()", 0) == 0) { cout << g.error() << endl; exit(EXIT_FAILURE); }   // (the ingest's word for it)
        die();
    }
    if (ranks.world > 1) {   // a rank without its graph or table says so to the others before they wait for it in the communicator
        auto say0 = [&](const std::string &what) {   // (one write per line: the ranks share the terminal)
            const std::string line = "rank " + std::to_string(ranks.rank) + ": " + what + "\n";
            if (write(2, line.data(), line.size()) < 0) {}
        };
        if (!g.good()) say0(g.error());
        if (!ranks.agree(g.good(), "load")) {
            if (g.good()) say0(ranks.err);
            if (ranks.rank == 0) (void)ranks.finish();
            _exit(EXIT_FAILURE);
        }
    }
    if (opt.auto_cutoffs) {   // as -h sets them from a histogram file (:354-358), with its checks
        opt.coverage_lower = max(10, cutoffL(counts.rows));
        opt.coverage_upper = cutoffH(counts.rows, opt.frequency);
        if (opt.coverage_lower < 0 || opt.coverage_upper < 0) { cerr << "Error: Filter coverage need a positive number." << endl; exit(EXIT_FAILURE); }
        if (opt.coverage_lower > opt.coverage_upper) { cerr << "Error: lower cutoff need be smaller than upper cutoff " << endl; exit(EXIT_FAILURE); }
    }
    if (!host_gfa) {
        cout << "CompactedDBG::read(): Graph loading successful" << endl;
        cout << "CDBG: Graph loading Real time : " << std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() << "s" << endl;
    }
    if (opt.verbose && graph.n_abundant)
        cout << "CompactedDBG::read(): " << graph.n_abundant << " k-length unitigs are abundant k-mers (numbered last, in Bifrost's hash table order)" << endl;
    // the single-sample path's settings and steps: shared with `ploidyfrost run` (pf_run_host.hpp)
    pfh::CallSetup call;
    call.outprefix = opt.outprefix;
    call.threads = opt.nb_threads;
    call.ref_threads = opt.ref_threads;
    call.lower = opt.coverage_lower;
    call.upper = opt.coverage_upper;
    call.info = opt.info;
    call.verbose = opt.verbose;
    call.model = model;
    call.filter = opt.filter_seen ? &filter : nullptr;
    call.density_points = dc.on ? dc.points : 0;
    call.density_adjust = dc.adjust;
    if (pfh::call_configure(g, call)) die();
    if (ranks.world > 1) {
        // ---- one graph over the GPUs of the node (the protocol of ploidyfrost_amd/dist.py from the C++ side) ----
        // every step that ends in a collective: the rank's own outcome first, then whether everybody is still there (pf_multi.hpp,
        // RankGroup::agree) -- a rank that failed alone must not leave the others waiting in RCCL
        // (one write per line: the ranks share the terminal)
        auto say = [&](const std::string &what) {
            const std::string line = "rank " + std::to_string(ranks.rank) + ": " + what + "\n";
            if (write(2, line.data(), line.size()) < 0) {}
        };
        auto leave = [&](const std::string &why) {
            say(why);
            if (ranks.rank == 0) (void)ranks.finish();
            _exit(EXIT_FAILURE);
        };
        auto together = [&](bool failed, const std::string &why, const char *stage) {
            if (failed) say(why);
            if (!ranks.agree(!failed, stage)) leave(failed ? std::string("leaving") : ranks.err);
        };
        if (!ranks.connect(g.device())) leave("--gpus: " + ranks.err);
        mark("communicator");
        g.set_write_super_bubble(ranks.rank == 0);
        int bad = 0;
        if (ranks.rank == 0) {
            bad = g.setUnitigId(opt.outprefix, opt.graphfile, opt.nb_threads);
            if (!bad && opt.info) bad = g.printInfo(opt.verbose, opt.outprefix);
        }
        if (!bad) bad = g.findSuperBubble_multithread_ptr(opt.outprefix, opt.nb_threads);   // every rank: the same state everywhere
        together(bad != 0, g.error(), "findSuperBubble");
        mark("findSuperBubble");
        cout << "CDBG:: Minimum Coverage:" << opt.coverage_lower << endl;
        cout << "CDBG:: Maximum Coverage:" << opt.coverage_upper << endl;
        const auto tp0 = std::chrono::steady_clock::now();
        cout << "CDBG::PloidyEstimation():  Analyzing superbubbles to generate sites' information" << endl;
        uint64_t nb = 0;
        bad = g.ploidy_select(opt.coverage_lower, opt.coverage_upper, nb);
        const uint64_t W = (uint64_t)ranks.world, R = (uint64_t)ranks.rank;
        const uint64_t t0b = nb / W * R + std::min<uint64_t>(R, nb % W), t1b = t0b + nb / W + (R < nb % W ? 1 : 0);
        uint64_t called = 0;
        if (!bad) bad = g.ploidy_align(t0b, t1b, called);
        together(bad != 0, g.error(), "align");
        std::vector<uint64_t> all((size_t)W * 18);
        if (!ranks.gather(g.device(), &called, 1, all.data())) leave("--gpus: " + ranks.err);
        uint64_t base = 0;
        for (uint64_t r = 0; r < R; ++r) base += all[r];
        uint64_t mine[18];
        bad = g.ploidy_text(base, mine, mine + PF_CALL_STREAMS);
        together(bad != 0, g.error(), "text");
        if (!ranks.gather(g.device(), mine, 18, all.data())) leave("--gpus: " + ranks.err);
        uint64_t offsets[PF_CALL_STREAMS] = {}, totals[PF_CALL_STREAMS] = {}, sums[8] = {};
        for (uint64_t r = 0; r < W; ++r) {
            for (int s_ = 0; s_ < PF_CALL_STREAMS; ++s_) {
                if (r < R) offsets[s_] += all[r * 18 + (uint64_t)s_];
                totals[s_] += all[r * 18 + (uint64_t)s_];
            }
            for (int c = 0; c < 8; ++c) sums[c] += all[r * 18 + PF_CALL_STREAMS + (uint64_t)c];
        }
        bad = g.ploidy_write(opt.outprefix, offsets, totals, true);
        together(bad != 0, g.error(), "write");
        uint64_t done = 1;   // nobody returns before everybody's slabs are in the files
        if (!ranks.gather(g.device(), &done, 1, all.data())) leave("--gpus: " + ranks.err);
        mark("PloidyEstimation");
        if (ranks.rank != 0) {
            fflush(nullptr);
            _exit(0);
        }
        printf("CDBG::PloidyEstimation():  Real time : %gs\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - tp0).count());
        printf("CDBG::PloidyEstimation(): Alleles in SuperBubbles  :\t2 :%llu\t3 :%llu\t4 :%llu\t5 :%llu\n", (unsigned long long)sums[0],
               (unsigned long long)sums[1], (unsigned long long)sums[2], (unsigned long long)sums[3]);
        if (sums[5]) printf("CDBG::PloidyEstimation(): Sites' Average Coverage:%d\n", (int)(sums[4] / sums[5]));
        if (opt.verbose) printf("[ranks]  %d ranks, %llu bubbles in the list, %llu called; this rank's slice %llu .. %llu\n", ranks.world, (unsigned long long)nb,
                                (unsigned long long)sums[6], (unsigned long long)t0b, (unsigned long long)t1b);
        cout.flush();
        fflush(nullptr);
        const int rc = ranks.finish();
        if (rc) { cerr << "a rank ended with status " << rc << endl; _exit(rc); }
        _exit(0);
    }
    if (pfh::call_run(g, call, mark)) die();
    // every result file is complete (PloidyEstimation joined the background writers): leave without walking the destructors
    cout.flush();
    cerr.flush();
    fflush(nullptr);
    mark("done");
    if (done_fd >= 0) {
        prctl(PR_SET_PDEATHSIG, 0);
        const unsigned char ok = 0;
        if (write(done_fd, &ok, 1) != 1) {}
        close(done_fd);
    }
    // (PF_ORDERLY_EXIT: leave through exit() -- a profiler that writes its report from an exit handler needs that)
    if (getenv("PF_ORDERLY_EXIT")) exit(0);
    _exit(0);
}
