/*
 * ploidyfrost_host.h -- C facade over the C++ host layer (pfh::UnitigSet + pfh::CDBG,
 * ploidyfrost_amd/csrc/host/pf_cdbg.hpp), so that non-C++ callers (bench.py, the tests) can
 * drive exactly the call sequence of the reference's main() (src/Main.cpp:829-849):
 *
 *   pfh_open(gfa, kmc_prefix, z, M, D, G, device)      CompactedDBG::read + CDBG::CDBG
 *   pfh_set_unitig_id(h, outpre)                       CDBG::setUnitigId
 *   pfh_find_superbubbles(h, outpre)                   CDBG::findSuperBubble_multithread_ptr
 *   pfh_ploidy_estimation(h, outpre, lower, upper)     CDBG::ploidyEstimation_multithread_ptr
 *
 * Everything compute-heavy inside runs on the GPU through ploidyfrost_hip.h.
 */
#ifndef PLOIDYFROST_HOST_H_
#define PLOIDYFROST_HOST_H_
#include <stdint.h>

#include "ploidyfrost_hip.h" /* pf_bfs_record */
#ifdef __cplusplus
extern "C" {
#endif

typedef struct pfh_run pfh_run;

typedef struct pfh_times {
    double load_s, upload_s;
    double bfs_device_s, replay_s, bubble_write_s, find_total_s;
    double cov_device_s, tasks_s, align_s, sites_s, format_s, write_s, ploidy_total_s;
    uint64_t unitigs, kmers, candidates, superbubbles, tasks, align_jobs, site_strings, output_bytes;
    uint64_t allele[4], core_cov, core_num;
    double scan_s, scan_serial_s; /* owner/order scan of PloidyEstimation: whole, and its sequential part */
    uint64_t bfs_large, bfs_max_seen; /* K-BFS traversals of more than 4096 vertices in the last findSuperBubble; the longest one */
    uint64_t bfs_deferred;            /* candidates that left the device's LDS tier (128 entries) for the host walkers */
    uint64_t snp_jobs, pair_jobs, wave_jobs; /* of align_jobs: bubbles finished by K-SNP, by K-PAIR, sent to K-BUBBLE (resident pipeline) */
    uint64_t stack_jobs;                     /* ... finished by K-STACK (paths of one length; the alignment certified to be the paths stacked) */
    uint64_t host_commit_records;            /* findSuperBubble: records committed on a host thread (large components, walked traversals) */
    uint64_t host_walk_vertices;             /* ... vertices the host walkers visited for the traversals the device gave up on */
} pfh_times;

/* NULL on failure: message via pfh_last_error(NULL) */
pfh_run *pfh_open(const char *gfa_path, const char *kmc_prefix, uint32_t complex_size, double match, double mismatch,
                  double gap, int device);
void pfh_close(pfh_run *);
const char *pfh_last_error(const pfh_run *);
void pfh_set_output_dir(pfh_run *, const char *dir); /* default ./PloidyFrost_output */
void pfh_set_write_files(pfh_run *, int on);         /* 0: format everything, write nothing */
void pfh_set_threads(pfh_run *, uint32_t threads);   /* host threads for the per-bubble phases (the reference's -t);
                                                         output order is always the -t 1 one */
void pfh_set_overlap_output(pfh_run *, int on);      /* 1: <outpre>_super_bubble.txt is written in the background and is complete
                                                         when pfh_ploidy_estimation (or pfh_close) returns; default 0 */
/* K-BFS traversals beyond 4096 vertices: on host cores (default, pf_bfs_candidates_split + host/pf_bfs_host.cpp: one thread per
 * traversal) or, with on = 0, on the device (k_bfs_huge: one wavefront per traversal).  Same records either way. */
void pfh_set_third_tier_on_host(pfh_run *, int on);
/* n > 1: write the text format of the reference's `-t n` functions (ids and var_count from 0, allele_frequency rows of a bubble
 * grouped by arity; src/CDBG.cpp:1829, 2056, 2158-2162, 2550) -- in the deterministic `-t 1` row order; n <= 1: the `-t 1` format.
 * Single-sample path. */
int pfh_set_reference_threads(pfh_run *, uint32_t n);
void pfh_set_batch_bubbles(pfh_run *, uint64_t n);
/* single-sample path: text pieces (4 x batch_bubbles bubbles, formatted / fetched / written one after the other) per alignment
 * launch; default 64 = the whole pass is aligned at once up to 2^24 bubbles.  Tests set small values to cross the boundaries. */
void pfh_set_align_pieces(pfh_run *, uint64_t n);   /* bubbles per batch of the align/format pipeline (default 65536) */
int pfh_set_unitig_id(pfh_run *, const char *outpre);
int pfh_find_superbubbles(pfh_run *, const char *outpre);
int pfh_ploidy_estimation(pfh_run *, const char *outpre, int lower, int upper);
/* ---- the coverage thresholds from the database itself (K-HIST, pf_count_histogram in ploidyfrost_hip.h) ----
 * pfh_kmc_histogram: the rows of the database's k-mer histogram, counted on the device from the decoded counters: row r = the number
 * of records whose count is *min_count + r, from the header's min_count through min(max_count, 2^(8 counter_size) - 1,
 * PF_HIST_MAX_BINS - 1), zero rows included; records outside [min_count, max_count] left out, counts above the cap in the last row.
 * (What `kmc_tools transform <db> histogram` writes as far as can be read without the tool: PARITY UNPINNED.)  At most cap rows are
 * copied, *n_rows = how many there are.  0 = ok, else pfh_last_error(NULL).
 * pfh_cutoffs_from_rows: cutoffL / cutoffH of src/Main.cpp:200-277 on the second column of a histogram, in file order: *lower = the
 * value before the callers' max(10, .), *upper = cutoffH at `quantile`.  0 = ok, 1 = fewer than two rows (the reference's "Histogram
 * File is badly Formatted."; *lower is set, *upper is not), 2 = a missing argument.  No device involved.
 * pfh_set_auto_cutoffs: the run derives its thresholds from its own database(s) -- a colored run one pair per colour -- on its
 * device context: max(10, lower), upper at `quantile`, with the checks of -h (lower <= upper); pfh_ploidy_estimation /
 * pfh_ploidy_estimation_colored then use them instead of their arguments.  quantile < 0: off again.
 * pfh_cutoffs: the pairs the last estimation used (before one: those pfh_set_auto_cutoffs derived); returns how many there are and
 * copies at most cap of them. */
int pfh_kmc_histogram(const char *kmc_prefix, uint64_t *rows_out, uint64_t cap, uint64_t *n_rows, uint64_t *min_count);
int pfh_cutoffs_from_rows(const uint64_t *rows, uint64_t n, double quantile, int *lower, int *upper);
int pfh_set_auto_cutoffs(pfh_run *, double quantile);
uint32_t pfh_cutoffs(const pfh_run *, int *lower, int *upper, uint32_t cap);
/* ---- low-coverage k-mers masked in reads (K-MASK, pf_mask_reads / pf_mask_fastq in ploidyfrost_hip.h) ----
 * Step 2 of the reference's workflow (README; script/pipeline/3.filter: `kmc_tools filter -hm <db> <reads.fq> -ci<L> <out.fq>`) in one
 * call: the database is mapped and decoded once (K-KMC), with auto_lower its histogram gives the lower threshold max(10, cutoffL)
 * (K-HIST, as `cutoffL -d` prints it), the count table is built, and the inputs are streamed through pf_mask_fastq in chunks of
 * chunk_bytes (0: 256 MB; a record that straddles a chunk edge is carried, a chunk without a whole record grows by the next one) into
 * out_path, one input after the other, written under a temporary name and renamed at the end.  The rule: csrc/pf_mask_rule.hpp.
 * Refused by name, with the input's path and the 1-based record number, nothing left under out_path or the temporary name: a record
 * whose first line does not start with '@' or whose third does not start with '+', a quality line of another length than its
 * sequence line, a line count that is no multiple of four, FASTA (first byte '>'), gzip (1f 8b), out_path equal to an input.
 * up = 0xFFFFFFFF: no upper bound.  *lower_used = the lower threshold that was applied.  0 = ok, else pfh_last_error(NULL).
 * pfh_mask_read: the rule on one read with the counters given by the caller (counters[i] for window i of 0 .. n - k, what
 * CKMCFile::GetCountersForRead fills); out[0..n) = the masked read; returns the bytes that changed.  No device involved.
 * pfh_mask_index_fastq: the FASTQ index of a chunk on the host (lines, roles, format clauses of the same header): returns the clause
 * of the smallest offending record (0 = none; pfh_mask_clause_text names it), *bad_record its 0-based number, *bytes_used and
 * *n_records as pf_mask_fastq gives them; read_off / read_len (may be NULL, cap entries) receive the sequence lines. */
int pfh_mask_fastq(const char *db_prefix, const char *const *inputs, uint32_t n_inputs, const char *out_path, uint32_t low, uint32_t up,
                   int auto_lower, uint64_t chunk_bytes, int device, pf_mask_stats *stats, uint32_t *lower_used);
uint64_t pfh_mask_read(const char *seq, uint64_t n, uint32_t k, const uint32_t *counters, uint32_t low, uint32_t up, char *out);
int pfh_mask_index_fastq(const char *text, uint64_t n, int final, uint64_t *bytes_used, uint64_t *n_records, uint64_t *bad_record,
                         uint64_t *read_off, uint32_t *read_len, uint64_t cap);
const char *pfh_mask_clause_text(int clause);
/* ---- k-mers counted from reads (K-COUNT, pf_count_* and pf_kmc_encode in ploidyfrost_hip.h) ----
 * Step `2.kmc_db` of the reference's workflow (`kmc -ci1 -cs10000 -k25 @FILES kmc_sample tmp`) in one call: the FASTQ inputs are
 * streamed through pf_count_fastq in chunks of chunk_bytes (0: 256 MB; the chunk contract and the format refusals of pfh_mask_fastq),
 * the counters with ci <= c <= cx are given out as min(c, cs) (kmc's letters; defaults 2, 1000000000, 255), and <out_prefix>.kmc_pre /
 * .kmc_suf are written in the KMC1 layout under temporary names and renamed at the end.  hist (may be NULL): the histogram file of the
 * finished counters, byte for byte what `histogram -d <out_prefix>` writes.  initial_slots: 0 = twice the first chunk's bytes.  The
 * rule: csrc/pf_count_rule.hpp.  Refused by name before a device context exists: no input, no output, k outside 3 .. 31, ci < 1,
 * ci > cx, cs < 1, a cut-off above 2^32 - 1, FASTA, gzip, an output that is an input.  0 = ok, else pfh_last_error(NULL).
 * pfh_mask_fastq_counted: `mask -k`: pfh_mask_fastq without a database -- the inputs are counted first with these options, the finished
 * counters give the histogram (auto_lower) and the table, the inputs are streamed a second time through K-MASK; db_out (may be NULL):
 * the database is written as well.
 * The host's plain restatement of the rule, no device involved:
 * pfh_count_reads_host: counts the reads text[off[i] .. off[i] + len[i]) and applies the cut-offs; at most cap sorted (k-mer, count)
 * pairs are written, *n is their number; returns the refusal of the options (0 = none; pfh_count_cut_text names it), -1 when a counter
 * passed 2^32 - 1.
 * pfh_count_encode_kmc1: the bytes of the two files for sorted distinct k-mers, with lut_prefix_len and counter_bytes by the rule;
 * at most *_cap bytes are written, *pre_n / *suf_n are the sizes. */
int pfh_count_fastq(const char *const *inputs, uint32_t n_inputs, const char *out_prefix, uint32_t k, uint64_t ci, uint64_t cx, uint64_t cs,
                    int both_strands, const char *hist, uint64_t chunk_bytes, uint64_t initial_slots, int device, pf_count_stats *stats);
int pfh_mask_fastq_counted(const char *const *inputs, uint32_t n_inputs, const char *out_path, uint32_t k, uint64_t ci, uint64_t cx, uint64_t cs,
                           int both_strands, const char *db_out, uint32_t low, uint32_t up, int auto_lower, uint64_t chunk_bytes, int device,
                           pf_mask_stats *stats, uint32_t *lower_used);
int pfh_count_reads_host(const char *text, const uint64_t *off, const uint32_t *len, uint64_t n_reads, uint32_t k, int both_strands, uint64_t ci,
                         uint64_t cx, uint64_t cs, uint64_t *kmers_out, uint32_t *counts_out, uint64_t cap, uint64_t *n, pf_count_stats *stats);
int pfh_count_encode_kmc1(const uint64_t *kmers, const uint32_t *counts, uint64_t n, uint32_t k, uint64_t ci, uint64_t cx, uint64_t cs,
                          int both_strands, uint8_t *pre_out, uint64_t pre_cap, uint64_t *pre_n, uint8_t *suf_out, uint64_t suf_cap, uint64_t *suf_n);
uint32_t pfh_count_counter_bytes(uint64_t cx, uint64_t cs);
uint32_t pfh_count_lut_prefix_len(uint32_t k);
const char *pfh_count_cut_text(int clause);
/* ---- the compacted de Bruijn graph built from reads (K-UNITIG, pf_unitig_* in ploidyfrost_hip.h) ----
 * Step `4.bifrost` of the reference's workflow (`Bifrost build -i -d -k 25 -r sample_filtered.fq -o sample`) in one call: the FASTQ
 * inputs are counted as pfh_count_fastq counts them (every k-mer kept, both strands; the chunk contract and the format refusals of
 * pfh_mask_fastq), the sorted k-mers are compacted into unitigs on the device and <out_prefix>.gfa is written (under a temporary name,
 * renamed at the end).  g: the ML tag of the header, PFH_UNITIG_G_DEFAULT = Bifrost's default for k (0 is refused like any other g outside 1 .. k - 2).  The rule: csrc/pf_unitig_rule.hpp.  Refused by name
 * before a device context exists: no input, no output, k outside 3 .. 31, g outside 1 .. k - 2, FASTA, gzip, an output that is an
 * input.  counted / stats (may be NULL): what the count and the graph report.
 * [tests] pfh_unitig_build_host: the host's plain restatement on k-mers in any order (no device): at most cap bytes of the text are
 * written, *text_bytes is its size, stats_out = {distinct, unitigs, removed, unitigs_out, longest, bytes}; 1: bad k or no k-mers
 * array, 2: bad g.  pfh_unitig_no_room_text: the wording of the refusal of buffers that do not fit the free device memory. */
#define PFH_UNITIG_G_DEFAULT (-2147483647 - 1)
int pfh_build_fastq(const char *const *inputs, uint32_t n_inputs, const char *out_prefix, uint32_t k, int32_t g, int clip_tips, int del_isolated,
                    uint64_t chunk_bytes, uint64_t initial_slots, int device, pf_count_stats *counted, pf_unitig_stats *stats);
int pfh_unitig_build_host(const uint64_t *kmers, uint64_t n, uint32_t k, int32_t g, int clip_tips, int del_isolated, char *text_out, uint64_t cap,
                          uint64_t *text_bytes, uint64_t stats_out[6]);
const char *pfh_unitig_no_room_text(uint64_t need, uint64_t free_bytes, uint64_t n_kmers);
/* ---- reads to ploidy estimate in one process (`ploidyfrost run`; K-MASKCOUNT, pf_maskcount_* in ploidyfrost_hip.h) ----
 * Steps 2 to 5 of the reference's workflow for one sample on one device context: the inputs counted (pfh_count_fastq's count with
 * k / ci / cx / cs), L = max(10, cutoffL) and U = cutoffU(quantile) of the counted k-mers, the count table, the inputs streamed a
 * second time through pf_maskcount_fastq (low = L, up = mask_up), the k-mers of the masked reads compacted into unitigs
 * (pfh_build_fastq's graph), and the single-sample calling run over that graph and that table with L and U; the twelve
 * PloidyFrost_output/<out_prefix>_*.txt files, with model_source the model's result as well.  No masked reads, no database and no
 * graph file lie in between; db_out / gfa_out (may be NULL) write the database of `mask --db-out` and the file of `build`.  L is
 * printed on stdout.  The rule of the second pass: csrc/pf_run_rule.hpp.  Refused by name before a device context exists: no
 * input, no output, k outside 5 .. 31, g outside 1 .. k - 2, ci < 1, ci > cx, cs < 1, FASTA, gzip, an output that is an input.
 * 0 = ok, else pfh_last_error(NULL).
 * pfh_count_masked_host: the host's plain restatement of the second pass, no device involved -- counters[p] is the counter of the
 * window that starts at byte p of the text (read at window starts only); every window that survives the masking with [low, up] is
 * counted in canonical form; at most cap sorted (k-mer, count) pairs are written, *n is their number; stats_out = {reads, bases,
 * kmers, kmers_invalid, kmers_bad, kmers_kept}.  1: bad k. */
typedef struct pfh_run_options {
    uint32_t k;                      /* 25 */
    uint64_t ci, cx, cs;             /* 1, 1000000000, 10000 */
    int32_t g;                       /* PFH_UNITIG_G_DEFAULT */
    int clip_tips, del_isolated;     /* 1, 1 */
    uint64_t chunk_bytes, initial_slots;
    double quantile;                 /* 0.998 */
    uint32_t mask_up;                /* 0xFFFFFFFF: no upper bound on the masking */
    uint32_t complex_size;           /* 8 */
    double match, mismatch, gap;     /* 2, -1, -3 */
    uint32_t threads;                /* 1 */
    int model_source;                /* -1: no model; PF_MODEL_COV / PF_MODEL_FRE */
    int model_only;
    const char *db_out, *gfa_out;    /* may be NULL */
} pfh_run_options;
typedef struct pfh_run_stats {
    uint64_t reads, bases, kmers, bad, distinct, lower, upper, windows_bad, windows_kept, distinct_kept, unitigs, removed, unitigs_out, longest;
} pfh_run_stats;
void pfh_run_defaults(pfh_run_options *opt);
int pfh_run_fastq(const char *const *inputs, uint32_t n_inputs, const char *out_prefix, const pfh_run_options *opt, int device, pfh_run_stats *stats);
int pfh_count_masked_host(const char *text, const uint64_t *off, const uint32_t *len, uint64_t n_reads, uint32_t k, const uint32_t *counters,
                          uint32_t low, uint32_t up, uint64_t *kmers_out, uint32_t *counts_out, uint64_t cap, uint64_t *n, uint64_t stats_out[6]);
/* ---- reads of several samples to per-sample ploidy in one process (`ploidyfrost run-multi`, K-UNION and K-COLORSET) ----
 * pfh_run_multi_fastq: for n_samples samples (a sample is a colour, named names[c], in the order given) what n_samples times
 * `mask -k ... --auto-cutoffs --db-out`, one `build-multi -i -d` and the coloured calling run with --auto-cutoffs do with files between
 * them, on one device context (csrc/host/pf_runmulti_host.hpp; the rule: csrc/pf_runmulti_rule.hpp).  inputs: the files of sample 0,
 * then of sample 1, ...; n_inputs_of[c] of them belong to sample c.  opt: pfh_run_options (db_out: <db_out><c>.kmc_pre / .kmc_suf per
 * sample; gfa_out: <gfa_out>.gfa and <gfa_out>.bfg_colors); a model needs multi (the options of `filter-multi`; may be NULL without
 * one), each_color: one estimate per colour.  per_color (may be NULL): four numbers per sample -- lower, upper, distinct k-mers
 * counted, distinct k-mers of the masked reads.  Every L is printed on stdout.  Refused by name before a device context exists: what
 * pfh_run_fastq refuses, no sample, more than 1024, a sample without input, a name twice, a file in two samples.  0 = ok, else
 * pfh_last_error(NULL).
 * pfh_union_host: the host's plain restatement of K-UNION (pairwise rounds, an odd set carried), no device involved: out holds the sum
 * of n[] keys at least, *n_out the size of the union.  1: a set that is not ascending or holds a key twice (pfh_last_error(NULL)). */
typedef struct pfh_run_multi_stats {
    uint64_t colors, reads, bases, kmers, bad, distinct, windows_bad, windows_kept, distinct_kept, unitigs, removed, unitigs_out, longest, kmers_colored,
        kmers_unplaced, runs, overflow, color_bytes;
} pfh_run_multi_stats;
int pfh_run_multi_fastq(const char *const *names, const uint32_t *n_inputs_of, uint32_t n_samples, const char *const *inputs, const char *out_prefix,
                        const pfh_run_options *opt, const pf_filter_multi_opts *multi, int each_color, int device, pfh_run_multi_stats *stats,
                        uint64_t *per_color);
int pfh_union_host(const uint64_t *const *sets, const uint64_t *n, uint32_t n_sets, uint64_t *out, uint64_t *n_out);
/* ---- the coloured graph built from several files of reads (K-COLOR, pf_color_* in ploidyfrost_hip.h) ----
 * `Bifrost build -c -k 25 [-i] [-d] -r s0.fq -r s1.fq ... -o sample` in one call: pfh_build_fastq's graph of all inputs together with a
 * DA tag on every S line, and <out_prefix>.bfg_colors (format version 2; csrc/host/pf_bfg_write.hpp), every input one colour in the
 * order given, named by its path as given.  Both files are written under temporary names and renamed at the end: both or neither.
 * Refused by name: what pfh_build_fastq refuses, more than 1024 inputs, the same path twice, n_seeds outside 1 .. 255 (0: 31).
 * [tests] pfh_build_colored_host: the host's plain restatement (no device) from the reads of every colour -- reads[i], n_reads of them,
 * belongs to colour colour_of[i] (ascending); the two files' bytes (at most the caps are written, the sizes always),
 * graph_stats = pfh_unitig_build_host's six, color_stats = {colors, windows_colored, windows_unplaced, windows_bad, runs, overflow};
 * 1: bad k or arguments, 2: bad g, 3: bad n_seeds, 4: too many colours or a unitig too long for them.
 * pfh_bfg_colors_bytes: the bytes of the colour file from what pf_color_fetch gives.  pfh_color_no_room_text: the refusal's wording. */
int pfh_build_colored_fastq(const char *const *inputs, uint32_t n_inputs, const char *out_prefix, uint32_t k, int32_t g, int clip_tips, int del_isolated,
                            uint32_t n_seeds, uint64_t chunk_bytes, uint64_t initial_slots, int device, pf_count_stats *counted, pf_unitig_stats *stats,
                            pf_color_stats *colored, uint64_t *color_bytes, double times_out[6]);
int pfh_build_colored_host(const char *const *reads, const uint32_t *colour_of, uint64_t n_reads, uint32_t n_colors, const char *const *names, uint32_t k,
                           int32_t g, int clip_tips, int del_isolated, uint32_t n_seeds, char *gfa_out, uint64_t gfa_cap, uint64_t *gfa_bytes,
                           uint8_t *colors_out, uint64_t colors_cap, uint64_t *colors_bytes, uint64_t graph_stats[6], uint64_t color_stats[6]);
int pfh_bfg_colors_bytes(const uint64_t *heads, const uint32_t *m, const uint32_t *slot, const uint64_t *run_off, const uint32_t *runs, uint64_t n_lines,
                         uint32_t k, uint32_t n_seeds, const char *const *names, uint32_t n_colors, uint8_t *out, uint64_t cap, uint64_t *bytes);
const char *pfh_color_no_room_text(uint64_t need, uint64_t free_bytes, uint64_t n_colors, uint64_t n_kmers);
/* ---- reads quality-trimmed (K-TRIM, pf_trim_fastq / pf_trim_fastq_pair in ploidyfrost_hip.h) ----
 * Step `1.trim` of the reference's workflow (`trimmomatic PE -phred33 r1 r2 trim1 u1 trim2 u2 LEADING:10 TRAILING:10 SLIDINGWINDOW:3:20
 * MINLEN:50`) in one call.  The rule: csrc/pf_trim_rule.hpp (parity with Trimmomatic unpinned: the tool is not part of the build).
 * pfh_trim_fastq: single-ended -- the inputs, one after the other, streamed through pf_trim_fastq in chunks of chunk_bytes (0: 256 MB;
 * the chunk contract and the format refusals of pfh_mask_fastq) into out_path.  pfh_trim_fastq_pair: record r of in1 pairs with record
 * r of in2; out_paths = o1 u1 o2 u2 (both kept -> o1 / o2, file 1 alone -> u1, file 2 alone -> u2); each file keeps its own carry, and
 * a file that ends while the other still holds a whole record is refused by name with the record counts; stats[f]: file f.
 * trimlog (may be NULL): one line per record in input order (pairs: record r of file 1, then of file 2),
 * `<header without '@'> <kept length> <b> <e> <n - e>`, a dropped record `0 0 0 0`.  Every output is written under a temporary name
 * and renamed at the end; nothing is left under any name after a refusal.  Refused by name before a device context exists: the steps
 * (unknown kind, value out of range, more than 8, none), phred other than 33 or 64, no or unreadable input, FASTA, gzip, an output
 * that is an input, two outputs with the same path.  0 = ok, else pfh_last_error(NULL).
 * The host's plain restatement of the rule, no device involved:
 * pfh_trim_parse_step: one of Trimmomatic's words ("LEADING:10") into a step; returns the refusal (0 = none; pfh_trim_refusal_text
 * names it).  pfh_trim_read: the rule on one quality line: 1 = kept with [*begin, *end), 0 = dropped, -1 = the steps or phred are
 * refused (pfh_last_error(NULL)).  pfh_trim_fastq_chunk: what pf_trim_fastq gives for one chunk: returns the format clause of the
 * smallest offending record (0 = none; pfh_mask_clause_text names it), -1 = the steps are refused; out holds n + 1 bytes; rec_begin /
 * rec_len (may be NULL): cap entries. */
int pfh_trim_fastq(const char *const *inputs, uint32_t n_inputs, const char *out_path, const pf_trim_step *steps, uint32_t n_steps, uint32_t phred,
                   const char *trimlog, uint64_t chunk_bytes, int device, pf_trim_stats *stats);
int pfh_trim_fastq_pair(const char *in1, const char *in2, const char *const *out_paths, const pf_trim_step *steps, uint32_t n_steps, uint32_t phred,
                        const char *trimlog, uint64_t chunk_bytes, int device, pf_trim_stats *stats);
int pfh_trim_parse_step(const char *word, pf_trim_step *step);
const char *pfh_trim_refusal_text(int refusal);
int pfh_trim_read(const char *qual, uint64_t n, const pf_trim_step *steps, uint32_t n_steps, uint32_t phred, uint32_t *begin, uint32_t *end);
int pfh_trim_fastq_chunk(const char *text, uint64_t n, int final, const pf_trim_step *steps, uint32_t n_steps, uint32_t phred, char *out,
                         uint64_t *out_bytes, uint64_t *bytes_used, uint32_t *rec_begin, uint32_t *rec_len, uint64_t cap, uint64_t *n_records,
                         pf_trim_stats *stats, uint64_t *bad_record);
/* ---- adapters clipped in front of the steps: `--adapters` (K-CLIP, pf_clip_begin .. pf_clip_end in ploidyfrost_hip.h) ----
 * The rule: csrc/pf_clip_rule.hpp (parity with Trimmomatic's ILLUMINACLIP unpinned; overlaps below 16 in simple mode and IUPAC
 * letters in adapters are not built; palindrome mode: below).  pfh_reads_adapters(path, seed, score): the next pfh_trim_fastq or pfh_trim_fastq_pair of this
 * thread reads the adapter file (FASTA; names ending in /1 or /2 choose the file of a pair, names starting with Prefix are skipped and
 * counted), opens a clip on its context and clips every read before the steps; n_steps may then be 0; the call takes the switch back
 * (path NULL or "": no clipping).  The file and the values are refused by name before a device context exists, with the path and the
 * 1-based record.  pfh_reads_adapters_report: what that call reported -- usable adapters, skipped entries, the clip's statistics.
 * The host's plain restatement of the rule, no device involved:
 * pfh_clip_parse_adapters: the text of an adapter file into bases (upper case, at most bases_cap bytes are written: 64 * 128 always
 * suffice), adapter_off (room for 65) and side (room for 64); returns the refusal (0 = none; pfh_clip_refusal_text names it) with
 * *bad_record = the 1-based record (0: the file as a whole).  pfh_clip_read: one read of file file_side (1 or 2): *clip_end = n
 * untouched, 0 dropped; *scored = the candidates whose seed held; -1 = the adapters or values are refused (pfh_last_error(NULL)).
 * pfh_trim_fastq_chunk_clip: what pf_trim_fastq gives for one chunk while a clip is open (pfh_trim_fastq_chunk with adapters; clip:
 * the statistics of this chunk, in place file_side - 1). */
void pfh_reads_adapters(const char *path, uint32_t seed, uint32_t score);
void pfh_reads_adapters_report(uint32_t *adapters, uint32_t *skipped, pf_clip_stats *stats);
int pfh_clip_parse_adapters(const char *text, uint64_t n, char *bases, uint64_t bases_cap, uint32_t *adapter_off, uint8_t *side, uint32_t *n_adapters,
                            uint32_t *skipped, uint64_t *bad_record);
const char *pfh_clip_refusal_text(int refusal);
int pfh_clip_read(const char *seq, const char *qual, uint64_t n, const char *bases, const uint32_t *adapter_off, const uint8_t *side, uint32_t n_adapters,
                  uint32_t file_side, uint32_t seed, uint32_t score, uint32_t phred, uint32_t *clip_end, uint64_t *scored);
int pfh_trim_fastq_chunk_clip(const char *text, uint64_t n, int final, const pf_trim_step *steps, uint32_t n_steps, uint32_t phred, const char *bases,
                              const uint32_t *adapter_off, const uint8_t *side, uint32_t n_adapters, uint32_t file_side, uint32_t seed, uint32_t score, char *out,
                              uint64_t *out_bytes, uint64_t *bytes_used, uint32_t *rec_begin, uint32_t *rec_len, uint64_t cap, uint64_t *n_records,
                              pf_trim_stats *stats, pf_clip_stats *clip, uint64_t *bad_record);
/* ---- palindrome mode: `--adapter-pairs` (K-PALIN, pf_clip_begin_pairs in ploidyfrost_hip.h) ----
 * pfh_reads_adapter_pairs(pair_score, pair_min, keep_both), called behind pfh_reads_adapters: the next pfh_trim_fastq_pair,
 * pfh_run_fastq_trimmed or pfh_run_multi_fastq_trimmed of this thread also reads the Prefix<X>/1, Prefix<X>/2 entries of the file as prefix
 * pairs and clips every pair by both modes; a single-ended call or sample is refused by name (`--adapter-pairs needs -1 / -2`).
 * pfh_reads_adapters_pair_report: the prefix pairs and what K-PALIN counted in that call.  The host's plain restatement, no device:
 * pfh_clip_parse_adapter_pairs: pfh_clip_parse_adapters with the switch on -- the usable adapters (may be none) and the prefix pairs
 * (prefix_bases: 8 * 2 * 128 bytes always suffice; prefix_off: room for 17).  pfh_clip_pair: the two reads of one pair under both
 * modes: clip_end[f] = the final clip end of file f; clip / pairs: the statistics of this one pair.  pfh_trim_fastq_pair_chunk_clip:
 * what pf_trim_fastq_pair gives for one chunk of each file while a clip with prefix pairs is open (out: o1, u1, o2, u2; clip_end[f]:
 * the final clip ends, at most cap entries as rec_begin / rec_len). */
void pfh_reads_adapter_pairs(uint32_t pair_score, uint32_t pair_min, int keep_both);
void pfh_reads_adapters_pair_report(uint32_t *pairs, pf_clip_pair_stats *stats);
int pfh_clip_parse_adapter_pairs(const char *text, uint64_t n, char *bases, uint64_t bases_cap, uint32_t *adapter_off, uint8_t *side, uint32_t *n_adapters,
                                 char *prefix_bases, uint64_t prefix_cap, uint32_t *prefix_off, uint32_t *n_pairs, uint64_t *bad_record);
int pfh_clip_pair(const char *seq1, const char *qual1, uint64_t n1, const char *seq2, const char *qual2, uint64_t n2, const char *bases,
                  const uint32_t *adapter_off, const uint8_t *side, uint32_t n_adapters, const char *prefix_bases, const uint32_t *prefix_off, uint32_t n_pairs,
                  uint32_t seed, uint32_t score, uint32_t pair_score, uint32_t pair_min, int keep_both, uint32_t phred, uint32_t clip_end[2],
                  pf_clip_stats *clip, pf_clip_pair_stats *pairs);
int pfh_trim_fastq_pair_chunk_clip(const char *text1, uint64_t n1, const char *text2, uint64_t n2, int final, const pf_trim_step *steps, uint32_t n_steps,
                                   uint32_t phred, const char *bases, const uint32_t *adapter_off, const uint8_t *side, uint32_t n_adapters,
                                   const char *prefix_bases, const uint32_t *prefix_off, uint32_t n_pairs, uint32_t seed, uint32_t score, uint32_t pair_score,
                                   uint32_t pair_min, int keep_both, char *out[4], uint64_t out_bytes[4], uint64_t bytes_used[2], uint32_t *rec_begin[2],
                                   uint32_t *rec_len[2], uint32_t *clip_end[2], uint64_t cap, uint64_t *n_records, pf_trim_stats stats[2], pf_clip_stats *clip,
                                   pf_clip_pair_stats *pairs, uint64_t *bad_record);
/* ---- the read quality report: `ploidyfrost qc` and `--report` (K-QC, pf_qc_* in ploidyfrost_hip.h) ----
 * The rule, the words of a table and the text of the report: csrc/pf_qc_rule.hpp.  pfh_reads_report(path): the next pfh_trim_fastq,
 * pfh_trim_fastq_pair or pfh_run_fastq_trimmed of this thread writes the report of both stages to `path` beside its other outputs, every
 * other output being what it is without; the call takes the switch back (null or "": none).  pfh_run_fastq refuses it by name (no
 * trimming: `qc` reports on files as they are), pfh_run_multi_fastq* as not built.  pfh_qc_fastq: `qc` -- every file streamed on its
 * own, inputs1 to side 1, inputs2 to side 2, stage raw alone, the report written under a temporary name and renamed at the end; takes
 * the pfh_reads_gz switch.  The host's plain restatement, no device: pfh_qc_fastq_chunk adds one chunk of one file (file_side 1 or 2) to
 * the tables raw, kept (trimmed != 0: the steps, and with clip_open the simple adapters as pfh_clip_read takes them) and clip, each of
 * PF_QC_TABLE_WORDS / PF_QC_CLIP_WORDS words; it returns the clause of pfh_mask_index_fastq (0 = ok) or -1 for a refused argument.
 * pfh_qc_report_text: tables [side][stage][PF_QC_TABLE_WORDS], clip [side][PF_QC_CLIP_WORDS] or null; *len = the bytes of the text, of
 * which at most cap go to out.  pfh_qc_phred_hint: 33, 64 or 0 from the smallest quality byte and the number of reads that held one. */
void pfh_reads_report(const char *path);
/* Duplicate reads dropped (K-DEDUP, `--dedup`; the rule: csrc/pf_dedup_rule.hpp).  pfh_reads_dedup(on, bases, initial_slots): the next
 * pfh_trim_fastq[_pair], pfh_run_fastq[_trimmed] or pfh_run_multi_fastq[_trimmed] call of this thread runs with a dedup, as `--dedup
 * [--dedup-bases N] [--dedup-initial-slots N]` does -- one table per unit of the command (a `trim` command: all its inputs; `run`: all
 * -i files together, each pair on its own; `run-multi`: the same per sample); no step is needed beside it, and in run / run-multi it
 * turns trimming on as a step does.  pfh_reads_dedup_report: what that call found, summed over its units (max_copies and slots: the
 * largest).  The host's plain restatement, no device: pfh_dedup_key: the key of one unit (seq2 NULL, n2 0: a single read); bases 0 =
 * the whole read, else 16 .. 4096; -1 = refused (pfh_last_error(NULL)).  pfh_dedup_units: the keys (two words each) of the units of a
 * whole stream in order, participates (may be NULL: all) -> keep[i] (1 = stays: the first of its key, or takes no part) and the
 * statistics (slots and growths 0).  pfh_trim_fastq[_pair]_chunk_dedup: what pf_trim_fastq[_pair] gives for one chunk while a dedup is
 * open and no clip, given the keys of the units that took part before (seen_keys, two words each, repeats allowed); rec_keys
 * (may be NULL): two words per unit of the chunk, 0 0 for one that takes no part; at most cap entries per array.  n_steps may be 0. */
void pfh_reads_dedup(int on, uint32_t bases, uint64_t initial_slots);
void pfh_reads_dedup_report(pf_dedup_stats *stats);
int pfh_dedup_key(const char *seq1, uint64_t n1, const char *seq2, uint64_t n2 /* NULL, 0: single */, uint32_t bases, uint64_t key[2]);
int pfh_dedup_units(const uint64_t *keys, const uint8_t *participates, uint64_t n, uint8_t *keep, pf_dedup_stats *stats);
int pfh_trim_fastq_chunk_dedup(const char *text, uint64_t n, int final, const pf_trim_step *steps, uint32_t n_steps, uint32_t phred, uint32_t bases,
                               const uint64_t *seen_keys, uint64_t n_seen, char *out, uint64_t *out_bytes, uint64_t *bytes_used, uint32_t *rec_begin,
                               uint32_t *rec_len, uint64_t *rec_keys, uint64_t cap, uint64_t *n_records, pf_trim_stats *stats, uint64_t *bad_record);
int pfh_trim_fastq_pair_chunk_dedup(const char *text1, uint64_t n1, const char *text2, uint64_t n2, int final, const pf_trim_step *steps, uint32_t n_steps,
                                    uint32_t phred, uint32_t bases, const uint64_t *seen_keys, uint64_t n_seen, char *out[4], uint64_t out_bytes[4],
                                    uint64_t bytes_used[2], uint32_t *rec_begin[2], uint32_t *rec_len[2], uint64_t *rec_keys, uint64_t cap, uint64_t *n_records,
                                    pf_trim_stats stats[2], uint64_t *bad_record);
int pfh_qc_fastq(const char *const *inputs1, uint32_t n1, const char *const *inputs2, uint32_t n2, const char *report_path, uint32_t phred, uint64_t chunk_bytes,
                 int device);
int pfh_qc_fastq_chunk(const char *text, uint64_t n, int final, uint32_t phred, uint32_t file_side, int trimmed, const pf_trim_step *steps, uint32_t n_steps,
                       int clip_open, const char *bases, const uint32_t *adapter_off, const uint8_t *side, uint32_t n_adapters, uint32_t seed, uint32_t score,
                       uint64_t *raw, uint64_t *kept, uint64_t *clip, uint64_t *bytes_used, uint64_t *n_records, uint64_t *bad_record);
uint32_t pfh_qc_phred_hint(uint64_t min_byte, uint64_t reads);
int pfh_qc_report_text(const uint64_t *tables, const uint64_t *clip, uint32_t phred, char *out, uint64_t cap, uint64_t *len);
/* ---- raw reads to ploidy estimate in one process: step `1.trim` inside `run` / `run-multi` (K-TRIMCOUNT, pf_*_trimmed in ploidyfrost_hip.h) ----
 * The rule: csrc/pf_trimrun_rule.hpp.  pfh_run_fastq_trimmed: pfh_run_fastq on the raw reads -- both passes stream them and trim them on
 * the device on the way in, no trimmed file is written.  paired = 0: what `trim -i inputs... -o t.fq STEP...` followed by
 * `run -i t.fq` writes; paired != 0: the inputs alternate file 1, file 2, and the result is that of one
 * `trim -1 .. -2 .. -o1 t1 -u1 .. -o2 t2 -u2 ..` per pair followed by `run -i t1 -i t2 [-i t1' -i t2' ...]`: the records of a pair go on
 * only when both are kept, the unpaired survivors are never counted.  n_steps = 0 with paired = 0 is pfh_run_fastq.  per_unit (may be
 * NULL): the trimming statistics of the first pass, one entry for all single-ended inputs together, one entry per input file when
 * paired.  Refused by name before a device context exists, beside what pfh_run_fastq refuses: what K-TRIM refuses about steps and
 * phred, paired inputs without a step or in odd number, a file given twice (by name or as one file under two names).  After the stream
 * has started: the files of a pair that hold different numbers of records, with the counts.
 * pfh_run_multi_fastq_trimmed: pfh_run_multi_fastq likewise; paired_of[c] != 0: the inputs of sample c are pairs; steps and phred
 * hold for every sample.  per_input (may be NULL): one entry per input file (a single-ended sample's unit stands in its first entry).
 * The host's plain restatement of the hand-on rule, no device involved: pfh_trim_table_chunk / pfh_trim_table_chunk_pair give what
 * pf_trim_table_fastq / pf_trim_table_fastq_pair give for one chunk -- the table (at most cap entries per file are written, *n_reads
 * always), bytes_used, *n_records, the statistics; they return the format clause of the smallest offending record (0 = none;
 * pfh_trim_table_clause_text names it, the pair's "final chunks hold different numbers of records" among them), -1 = the steps are
 * refused. */
int pfh_run_fastq_trimmed(const char *const *inputs, uint32_t n_inputs, int paired, const pf_trim_step *steps, uint32_t n_steps, uint32_t phred,
                          const char *out_prefix, const pfh_run_options *opt, int device, pfh_run_stats *stats, pf_trim_stats *per_unit);
int pfh_run_multi_fastq_trimmed(const char *const *names, const uint32_t *n_inputs_of, const int *paired_of, uint32_t n_samples, const char *const *inputs,
                                const pf_trim_step *steps, uint32_t n_steps, uint32_t phred, const char *out_prefix, const pfh_run_options *opt,
                                const pf_filter_multi_opts *multi, int each_color, int device, pfh_run_multi_stats *stats, uint64_t *per_color,
                                pf_trim_stats *per_input);
int pfh_trim_table_chunk(const char *text, uint64_t n, int final, const pf_trim_step *steps, uint32_t n_steps, uint32_t phred, uint64_t *read_off,
                         uint32_t *read_len, uint64_t cap, uint64_t *n_reads, uint64_t *bytes_used, uint64_t *n_records, pf_trim_stats *stats,
                         uint64_t *bad_record);
int pfh_trim_table_chunk_pair(const char *text1, uint64_t n1, const char *text2, uint64_t n2, int final, const pf_trim_step *steps, uint32_t n_steps,
                              uint32_t phred, uint64_t *const read_off[2], uint32_t *const read_len[2], uint64_t cap, uint64_t *n_reads, uint64_t bytes_used[2],
                              uint64_t *n_records, pf_trim_stats stats[2], uint64_t *bad_record);
const char *pfh_trim_table_clause_text(int clause);
void pfh_get_times(const pfh_run *, pfh_times *out);
/* Where the loads of this process spent their time (GFA map / parse / upload, count database, join, adjacency, numbering, ...):
 * "step\tseconds\n" per step since the last reset, in the order the steps ended (steps of helper threads overlap those of the
 * caller's).  Returns the length of the text; at most cap - 1 bytes and a NUL are written.  reset != 0 empties the log afterwards. */
uint64_t pfh_load_trace(char *out, uint64_t cap, int reset);
/* The row filters behind the path (reference script/Filter.R, script/Filter-multi.R; csrc/host/pf_filter.hpp; PARITY UNPINNED --
 * no R in the build image): argv as the scripts take it (argv[0], argv[1] are skipped like "ploidyfrost filter"), multi != 0 = the
 * colored tables.  pfh_r_format_double: one number as R's write.table renders it (15 significant digits, fixed or scientific by
 * width); returns the length, writes at most cap - 1 bytes and a NUL. */
int pfh_filter(int argc, char **argv, int multi);
uint64_t pfh_r_format_double(double x, char *out, uint64_t cap);
/* the pf_ctx of include/ploidyfrost_hip.h that this run drives (timing, stream control) */
void *pfh_device_ctx(pfh_run *);
/* <outpre>_allele_frequency.txt of the last pfh_ploidy_estimation, in memory (valid until the next
 * run): the per-rank record slab that a multi-GPU job all-gathers. */
const char *pfh_last_allele_frequency(const pfh_run *, uint64_t *len);
/* per-unitig state after pfh_find_superbubbles (MyUnitig flag byte, partner ids; 0 = NULL) */
void pfh_state(const pfh_run *, uint8_t *flags, uint32_t *plus, uint32_t *minus);

/* ---- colored (multi-sample) runs: the call sequence of src/Main.cpp:775-810 --------------------------
 *   pfh_open_colored(gfa, bfg_colors, kmc_list, ...)          ColoredCDBG::read + CCDBG::CCDBG
 *   pfh_set_unitig_id / pfh_find_superbubbles                 CCDBG::setUnitigId / findSuperBubble_multithread_ptr
 *   pfh_ploidy_estimation_colored(h, outpre, lower, upper, n) CCDBG::ploidyEstimation_multithread_ptr, one
 *                                                             (lower, upper) cutoff per colour (the -C file)
 * kmc_list_file: one KMC database prefix per line, one line per colour (src/CCDBG.cpp:13-43). */
pfh_run *pfh_open_colored(const char *gfa_path, const char *colors_path, const char *kmc_list_file, uint32_t complex_size,
                          double match, double mismatch, double gap, uint32_t threads, int device);
uint32_t pfh_num_colors(const pfh_run *);
int pfh_ploidy_estimation_colored(pfh_run *, const char *outpre, const int *lower, const int *upper, uint32_t n_colors);

/* ---- colour sets of a colored graph (no GPU involved) -----------------------------------------
 * The product's own reader of Bifrost's .bfg_colors (ploidyfrost_amd/csrc/host/pf_host_colors.hpp), which
 * replaces ColoredCDBG::read -> DataStorage::read -> UnitigColors::read (bifrost/src/ColoredCDBG.tcc:428,
 * DataStorage.tcc:790, ColorSet.cpp:1228) on the CCDBG path.  Exposed so that tests can hold it against
 * the real Bifrost's reading of the same file. */
typedef struct pfh_colors pfh_colors;
pfh_colors *pfh_colors_open(const char *gfa_path, const char *colors_path, uint32_t threads); /* NULL: pfh_last_error(NULL) */
void pfh_colors_close(pfh_colors *);
uint32_t pfh_colors_count(const pfh_colors *);                 /* ColoredCDBG::getNbColors */
uint32_t pfh_colors_unitigs(const pfh_colors *);
const char *pfh_colors_name(const pfh_colors *, uint32_t colour);
/* presence[colour * n_kmers + i] = 1 when k-mer i (reference orientation) of unitig u carries the colour
 * (UnitigColors::contains, ColorSet.cpp:776); returns UnitigColors::size(um) (ColorSet.cpp:898);
 * *n_full_enc = colours the file stores in the {full colours, rest} pair form, 0 otherwise */
uint64_t pfh_colors_unitig(const pfh_colors *, uint32_t u, uint8_t *presence, uint32_t *n_kmers, uint32_t *n_full_enc);
/* The unitig numbering is the reference's `-t 1` one: long unitigs in S-line order, then k-length unitigs in S-line
 * order, then the k-length unitigs Bifrost files as "abundant" k-mers (their minimizer's bucket already held 15 entries
 * when they were read, CompactedDBG.tcc:4013-4021, 4031-4068) in the slot order of its k-mer hash table
 * (KmerHashTable.hpp:326-354; UnitigIterator.tcc:32-58).
 * pfh_gfa_abundant_kmers: how many unitigs of the file end up in that last group (UINT64_MAX = unreadable file).
 * pfh_gfa_write_unitig_ids: writes `id<TAB>sequence` per unitig, the content of <prefix>_Unitig_Id.txt (src/CDBG.cpp:121-143),
 * from the GFA file alone (no device involved); 0 = ok.
 * pfh_gfa_numbering_replays: 0 when no minimizer bucket can reach 15 entries (nothing to decide), else how many times the
 * loader replayed Bifrost's bucket bookkeeping (> 1: long unitigs were redirected into buckets it had not followed). */
uint64_t pfh_gfa_abundant_kmers(const char *gfa_path);
uint32_t pfh_gfa_numbering_replays(const char *gfa_path);
/* the host pass's saturating minimizer-occurrence counters (what K-MINZ, pf_minimizer_crowding, bounds from above): returns
 * the number of slots (0 when the graph has no k-length unitig to decide about) and fills counters when slots suffices */
uint64_t pfh_gfa_minimizer_counts(const char *gfa_path, uint8_t *counters, uint64_t slots);
int pfh_gfa_write_unitig_ids(const char *gfa_path, const char *out_path);
/* [tests] the same file through the numbering replay with its inputs handed in (as pf_minimizer_replay_inputs hands them over): the host's
 * own counters + bump (saturating upper bounds), every unitig flagged */
int pfh_gfa_write_unitig_ids_given_inputs(const char *gfa_path, const char *out_path, int bump);
/* [tests] the same with the two arrays of pf_minimizer_replay_inputs themselves: n_slots saturating counters and one flag per unitig
 * in the loader's order before the move (segments longer than k in file order, then the k-length ones).  Non-zero, with a message
 * under pfh_last_error(NULL), when n_slots is not the table size of this graph or n_flags not its number of unitigs: the arrays
 * are used as handed in or not at all */
int pfh_gfa_write_unitig_ids_given_arrays(const char *gfa_path, const char *out_path, const uint8_t *counters8, uint64_t n_slots,
                                          const uint8_t *flags, uint64_t n_flags);
/* ---- `PloidyFrost model`: class GmmModel (src/GmmModel.hpp:5-49) and the driver of src/Main.cpp:636-692 ------------------
 * pfh_gmm_open needs no device; the readers are the reference's text parsers (readFreFile src/GmmModel.cpp:240-257,
 * readCovFile :21-239); pfh_gmm_fit = setMThreshold/setNThreshold/setMaxIterNum/setMaxDeltaNum + resize(gauss) +
 * emIterate() on the GPU (fails without one); pfh_gmm_run fits gauss = min..max and writes <outprefix>_model_result.txt
 * (Main.cpp:659-690).  Every call: 0 = ok, else pfh_gmm_last_error(). */
typedef struct pfh_gmm pfh_gmm;
pfh_gmm *pfh_gmm_open(int device);
void pfh_gmm_close(pfh_gmm *);
const char *pfh_gmm_last_error(const pfh_gmm *);
int pfh_gmm_read_fre(pfh_gmm *, const char *allele_frequency_file, double min_frequency);
int pfh_gmm_read_cov(pfh_gmm *, const char *coverage_file_prefix, double min_frequency);
int pfh_gmm_set_values(pfh_gmm *, const double *values, uint64_t n);   /* GmmModel::readData */
uint64_t pfh_gmm_size(const pfh_gmm *);
int pfh_gmm_values(const pfh_gmm *, double *out);
int pfh_gmm_fit(pfh_gmm *, uint32_t gauss, double m_thre, double n_thre, int32_t max_iter, double max_delta, double *weights,
                double *means, double *vars, double *loglik, double *aic, uint32_t *iterations);
int pfh_gmm_run(pfh_gmm *, int min_gauss, int max_gauss, double m_thre, double n_thre, int32_t max_iter, double max_delta,
                const char *outprefix);
/* enable = 1 / 0 switches the HIP-event timing of the K-GMM launches on / off; enable < 0 reads the totals */
int pfh_gmm_kernel_time(pfh_gmm *, int enable, double *total_ms, uint64_t *launches);
/* ---- the curve script/Drawfreq.R draws, as numbers (pf_gmm_density in ploidyfrost_hip.h) ----
 * pfh_gmm_read_column: a plain column of numbers, what Drawfreq's read.table makes of its -f file (blank lines and lines that begin
 * with '#' skipped; every other line one finite number that strtod consumes whole, else refused with the line number; no frequency
 * test, no doubled last value).  pfh_gmm_density: the Gaussian kernel density of the model's values on the GPU by ggplot2's
 * geom_density defaults (x, density: `points` doubles each); the exact sum, where R's density() bins onto 1024 cells and convolves by
 * FFT -- parity with R is unpinned.  Fewer than two values: "need at least 2 data points".  pfh_gmm_write_density writes
 * <outprefix>_allele_frequency_density.txt: the line "# values N bandwidth BW points P", then P rows x<TAB>density, every number
 * %.17g (the doubles exactly).  pfh_gmm_density_time: the HIP-event time of the density launches since timing was switched on
 * (pfh_gmm_kernel_time with enable = 1). */
int pfh_gmm_read_column(pfh_gmm *, const char *column_file);
int pfh_gmm_density(pfh_gmm *, uint32_t points, double adjust, double *x, double *density, pf_density_info *info);
int pfh_gmm_write_density(pfh_gmm *, const char *outprefix, const pf_density_info *info, uint32_t points, const double *x, const double *density);
int pfh_gmm_density_time(pfh_gmm *, double *total_ms, uint64_t *launches);

/* ---- the ploidy estimate in the same run (single-sample path; pf_call_model_* in ploidyfrost_hip.h) ----
 * pfh_set_model before pfh_ploidy_estimation: that call then feeds the model from the text pieces while they are resident on the
 * device, fits gauss = lo .. hi on the run's own context and writes <outpre>_model_result.txt -- the bytes
 * `model -f <outpre>` (source 0, cov) / `model -g <outpre>_allele_frequency.txt` (source 1, fre) write from the files.
 * source < 0 switches it off again.  only != 0: none of the ten calling files is written and none of their text is copied to the
 * host.  Options as `PloidyFrost model` checks them (q < 0.5, 1 <= lo <= hi <= PF_GMM_MAX_GAUSS, the rest >= 0); refused for a
 * colored run.  0 = ok, else pfh_last_error().
 * After the pass: pfh_model_values copies min(cap, n) values of the device array and returns n; pfh_model_fit returns the record of
 * `gauss` Gaussians (arrays of gauss doubles; 0 = ok, 1 = no such fit); pfh_model_ploidy the value of the result file's last line
 * (0 when nothing was fitted); pfh_text_bytes_fetched how many bytes of the ten calling streams that pass copied from the device. */
int pfh_set_model(pfh_run *, int source, double min_frequency, int lo, int hi, double m_thre, double n_thre, int32_t max_iter,
                  double max_delta, int only);
uint64_t pfh_model_values(pfh_run *, double *out, uint64_t cap);
int pfh_model_fit(const pfh_run *, uint32_t gauss, double *weights, double *means, double *vars, double *loglik, double *aic,
                  uint32_t *iterations);
double pfh_model_ploidy(const pfh_run *);
/* pfh_set_density after pfh_set_model: the pass then takes the kernel density (pf_gmm_density) of the array each fit reads, right
 * after that fit -- the pooled array, and split by colour every colour's -- and writes <outpre>_allele_frequency_density.txt /
 * <outpre>_color<c>_allele_frequency_density.txt beside the model results.  points == 0 switches it off, as switching the model off
 * does; refused without a model, for points outside PF_DENSITY_MIN_POINTS .. PF_DENSITY_MAX_POINTS and for an adjust that is not a
 * finite positive number.  After the pass: pfh_model_density_points(color < 0: pooled) = the grid's length (0: no curve),
 * pfh_model_density / pfh_model_color_density copy grid, curve and record (each may be NULL; 0 = ok, 1 = no curve). */
int pfh_set_density(pfh_run *, uint32_t points, double adjust);
uint32_t pfh_model_density_points(const pfh_run *, int color);
int pfh_model_density(const pfh_run *, double *x, double *density, pf_density_info *info);
int pfh_model_color_density(const pfh_run *, int color, double *x, double *density, pf_density_info *info);
uint64_t pfh_text_bytes_fetched(const pfh_run *);
/* The row rule of that path on text in host memory (csrc/pf_model_rows.hpp, the code the device kernels run), no device involved:
 * source 0: text[0..2] = the bytes of _bicov / _tricov / _tetracov.txt, source 1: text[0] = those of _allele_frequency.txt; the
 * values in file order to out (at most cap; *n = how many there are).  0 = ok, 1 = an error of the readers (a coverage row that
 * sums to 0, a token that is no number) or a number the rule does not convert exactly, worded in err. */
int pfh_model_rows(int source, double min_frequency, const char *const *text, const uint64_t *len, double *out, uint64_t cap,
                   uint64_t *n, char *err, uint64_t err_cap);

/* ---- `ploidyfrost filter`'s row predicates in front of that model (pf_filter_opts and pf_call_model_filter in ploidyfrost_hip.h) ----
 * pfh_set_filter after pfh_set_model: the next pfh_ploidy_estimation fits what `filter -i <outpre> ...` followed by `model -f` /
 * `model -g <filtered>_allele_frequency.txt` would read, from the coverage text while it is on the device; no filtered table is
 * written.  NULL: no filter again.  Refused (pfh_last_error) unless a model is set and for frequency > 0.5; pfh_set_model with
 * source < 0 drops the filter as well.  When no table keeps a row the pass fails with R's error after the calling files are
 * complete, and the run stays usable.
 * pfh_filter_rows: the same rule (csrc/pf_filter_rows.hpp) on host text, no device: text[0..3] = the bytes of _bicov / _tricov /
 * _tetracov / _pentacov.txt, out = the model's array for `source` (at most cap; *n = how many there are).  0 = ok, 1 = refused,
 * worded in err as the device path words it. */
int pfh_set_filter(pfh_run *, const pf_filter_opts *);
int pfh_filter_rows(int source, double min_frequency, const pf_filter_opts *opts, const char *const *text, const uint64_t *len,
                    double *out, uint64_t cap, uint64_t *n, char *err, uint64_t err_cap);

/* ---- the colored path: `ploidyfrost filter-multi`'s predicates in front of the model (pf_filter_multi_opts in ploidyfrost_hip.h) ----
 * A colored run accepts pfh_set_model behind a multi filter only (its unfiltered tables pool every sample): pfh_set_model, then
 * pfh_set_filter_multi, then pfh_ploidy_estimation_colored, which fits what `filter-multi -i <outpre> ...` followed by `model`
 * would read and writes no filtered table.  each_color != 0 (with opts->color < 0): one fit for every colour that keeps a row, in
 * colour order, written to <outpre>_color<c>_model_result.txt -- the chain run with -c c -- and no pooled result file;
 * pfh_model_values then gives the pooled array (of the last pass, whatever is set afterwards); a colour whose kept rows hold no
 * value for the model is not fitted and gets no file, and the colours above it are fitted all the same.  NULL: off again, as pfh_set_model with source < 0 does.  Refused on a
 * single-sample run, without a model, for frequency > 0.5 and for each_color with one colour; pfh_set_filter is refused on a
 * colored run; a colored pass with a model and no multi filter is refused when it starts.
 * After a pass split by colour: pfh_model_color_count = the colours fitted, pfh_model_color_at(i) the i-th of them (ascending);
 * pfh_model_color_values / _fit / _ploidy as pfh_model_values / _fit / _ploidy for one colour (values: ~0 for a colour without a
 * fit; fit: 1).
 * pfh_filter_rows_multi: the multi rule on host text as pfh_filter_rows has the single-sample one (rows of A + 7 fields). */
int pfh_set_filter_multi(pfh_run *, const pf_filter_multi_opts *, int each_color);
int pfh_filter_rows_multi(int source, double min_frequency, const pf_filter_multi_opts *opts, const char *const *text, const uint64_t *len,
                          double *out, uint64_t cap, uint64_t *n, char *err, uint64_t err_cap);
uint32_t pfh_model_color_count(const pfh_run *);
int pfh_model_color_at(const pfh_run *, uint32_t i);
uint64_t pfh_model_color_values(const pfh_run *, int color, double *out, uint64_t cap);
int pfh_model_color_fit(const pfh_run *, int color, uint32_t gauss, double *weights, double *means, double *vars, double *loglik, double *aic,
                        uint32_t *iterations);
double pfh_model_color_ploidy(const pfh_run *, int color);

/* The host tier of K-BFS on its own (host/pf_bfs_host.hpp; no device involved): extractSuperBubble_ptr's traversal
 * (src/CDBG.cpp:253-372) from one oriented vertex over CSR rows laid out as pf_build_adjacency returns them.  Fills *record
 * (list_off = 0) and copies its list -- seen[] when an exit was found, the cycle set otherwise -- to `list`.
 * 0 = ok, 2 = list_cap too small (record->n_list says how much is needed). */
int pfh_host_walk(const uint32_t *succ, const uint32_t *pred, uint32_t n_unitigs, uint32_t entrance, pf_bfs_record *record, uint32_t *list,
                  uint64_t list_cap);

/* ---- one graph over several GPUs: every rank opens the same graph and database -------------------------------
 * findSuperBubble:   pfh_find_shard(u0, u1) traverses the candidate entrances on this rank's unitig range (K-BFS + host walkers);
 *                    pfh_shard_records / pfh_shard_pool expose the records (pf_bfs_record, list_off relative to the pool) for the
 *                    exchange (RCCL all-gather); pfh_find_replay applies the records of all shards in shard order -- the
 *                    reference's visiting order with its `partner == NULL` gate (src/CDBG.cpp:206-214) -- so that every rank ends
 *                    with the same MyUnitig state; write_file = 1 on the rank that writes <outpre>_super_bubble.txt.
 * PloidyEstimation:  pfh_ploidy_select (scan + sequential pass, on every rank) -> n_bubbles, the run's bubble list in output
 *                    order; the rank aligns its contiguous slice [t0, t1) (pfh_ploidy_align -> how many of them are called:
 *                    var_count, src/CDBG.cpp:1254-1258); after exchanging those counts it formats with the number of bubbles
 *                    called by the ranks before it (pfh_ploidy_text -> the byte sizes of its ten slabs and counters[8] =
 *                    {2,3,4,5-allele sites, coreCov, coreNum, called, bubbles}); after exchanging the sizes it writes its slabs at
 *                    its offsets of the shared result files (pfh_ploidy_write; truncate = 1 cuts them to `totals`: pass it on
 *                    every rank, the length is the same).  Rank-order concatenation = the reference's `-t 1` files, because a
 *                    bubble's position is fixed by its owner endpoint (:1190, 1352, 1656-1679). */
int pfh_find_shard(pfh_run *, uint32_t u0, uint32_t u1);
const pf_bfs_record *pfh_shard_records(const pfh_run *, uint64_t *n_records);
const uint32_t *pfh_shard_pool(const pfh_run *, uint64_t *n_entries);
/* pool_lens (entries of each pool; NULL = sequential replay): the commits run on host threads, component by component
 * (pfh_set_replay_threads; csrc/host/pf_replay_par.hpp), the components found on the device -- from dev_records / dev_pools when the
 * shards already lie in device memory (the all-gather's output), else from an upload of records / pools. */
int pfh_find_replay(pfh_run *, const char *outpre, uint32_t n_shards, const pf_bfs_record *const *records, const uint64_t *n_records,
                    const uint32_t *const *pools, int write_file, const uint64_t *pool_lens, const pf_bfs_record *const *dev_records,
                    const uint32_t *const *dev_pools);
/* where the commits of findSuperBubble run: -1 = default (single-sample path: on the device, one thread per component,
 * pf_replay_device; pfh_find_replay and the colored path: host threads / sequential), 0 = the sequential loop on the host,
 * n >= 2 = n host threads, component by component */
void pfh_set_replay_threads(pfh_run *, int threads);
/* several ranks running findSuperBubble on the same graph into one output directory: 0 on all but the rank that writes
 * <outpre>_super_bubble.txt (the rows are computed everywhere; PloidyEstimation does not need the file) */
void pfh_set_write_super_bubble(pfh_run *, int on);
int pfh_ploidy_select(pfh_run *, int lower, int upper, uint64_t *n_bubbles);
/* the same for a colored run (pfh_open_colored): one (lower, upper) per colour, the reference's -C file (src/Main.cpp:775-810) */
int pfh_ploidy_select_colored(pfh_run *, const int *lower, const int *upper, int n_cutoffs, uint64_t *n_bubbles);
int pfh_ploidy_align(pfh_run *, uint64_t t0, uint64_t t1, uint64_t *n_called);
int pfh_ploidy_text(pfh_run *, uint64_t var_count_base, uint64_t sizes[10], uint64_t counters[8]);
int pfh_ploidy_write(pfh_run *, const char *outpre, const uint64_t offsets[10], const uint64_t totals[10], int truncate);

/* The same exchange without a device (CPU tests of the N > 1 path): the records of a unitig range from the host walker alone
 * (pfh_host_walk_range: every oriented vertex with out-degree > 1 on unitigs [u0, u1), ascending; returns the number of records,
 * *pool_used the list entries; UINT64_MAX when a capacity is too small) and the commit replay on a bare state
 * (pfh_replay_open: n_unitigs, -z; pfh_replay_apply: one shard's records, in shard order; pfh_replay_state as pfh_state). */
uint64_t pfh_host_walk_range(const uint32_t *succ, const uint32_t *pred, uint32_t n_unitigs, uint32_t u0, uint32_t u1,
                             pf_bfs_record *records, uint64_t rec_cap, uint32_t *pool, uint64_t pool_cap, uint64_t *pool_used);
typedef struct pfh_replay pfh_replay;
pfh_replay *pfh_replay_open(uint32_t n_unitigs, uint32_t complex_size);
void pfh_replay_close(pfh_replay *);
int pfh_replay_apply(pfh_replay *, const pf_bfs_record *records, uint64_t n_records, const uint32_t *pool);
void pfh_replay_state(const pfh_replay *, uint8_t *flags, uint32_t *plus, uint32_t *minus);
/* The same replay spread over `threads` host threads: records whose footprints (the unitig sides they can touch) are disjoint
 * commute, so the connected components of {sides, "touched by one record"} are replayed side by side, each in record order
 * (csrc/host/pf_replay_par.hpp).  A handle takes either this call or pfh_replay_apply.  pfh_side_components: the component
 * label of every record's entrance side (what pf_side_components computes on the device); pfh_replay_check_footprints: the
 * sequential replay with every state access checked against those components, `slice` records at a time (0 = all at once)
 * -> number of accesses outside the running record's component (0 = the model holds), *first_bad = the first such record. */
int pfh_replay_apply_parallel(pfh_replay *, const pf_bfs_record *records, uint64_t n_records, const uint32_t *pool, uint32_t threads);
void pfh_side_components(const pf_bfs_record *records, uint64_t n_records, const uint32_t *pool, uint32_t n_unitigs, uint32_t *labels);
uint64_t pfh_replay_check_footprints(const pf_bfs_record *records, uint64_t n_records, const uint32_t *pool, uint32_t n_unitigs,
                                     uint32_t complex_size, uint64_t slice, uint64_t *first_bad);
/* the same with the colored commits (CCDBG): colour sets of an opened (graph, colours) pair, succ = the graph's CSR rows [2N][4] */
struct pfh_colors;
uint64_t pfh_colors_check_footprints(const struct pfh_colors *, const uint32_t *succ, const pf_bfs_record *records, uint64_t n_records,
                                     const uint32_t *pool, uint32_t complex_size, uint64_t slice, uint64_t *first_bad);

/* ---- blocked gzip (K-INFLATE, `--gz`): the rule without a device (csrc/pf_inflate_rule.hpp) ----
 * Every call returns a clause of pf_inflate::Clause (0 = none), worded by pfh_inflate_clause_text.
 * pfh_inflate_parse_member: one BGZF member header at bytes[0, n), n = bytes up to the end of the file;
 *   fields = { payload offset 12 + XLEN, member length BSIZE + 1, CRC32, ISIZE }.
 * pfh_inflate_member: one member's deflate stream payload[0, n_in) -> out[0, isize); nothing outside either range is touched whatever
 *   the bytes say.  *produced = bytes written, blocks = { stored, fixed, dynamic }.  The CRC is not looked at.
 * pfh_inflate_bgzf_member: a whole member: header, stream, length and CRC-32; out holds 65536 bytes.
 * pfh_inflate_crc32 / _sliced: the CRC-32 of n bytes, plainly and from `n_lanes` slices as the kernel's lanes compute it.
 * pfh_inflate_file_clause: what the first bytes of a file say with `--gz`: 0 plain, 1 blocked gzip, 2 refused with *clause. */
/* `--gz` for the calls that take the sequencer's files: after pfh_reads_gz(1) the next pfh_count_fastq, pfh_trim_fastq[_pair],
 * pfh_run_fastq[_trimmed] or pfh_run_multi_fastq[_trimmed] of this thread reads inputs with the gzip magic as blocked gzip and inflates
 * them on the device; the call takes the switch back.  (pfh_trim_read and pfh_trim_fastq_chunk, which build the same options, take it
 * back as well and ignore it.) */
void pfh_reads_gz(int on);
/* `--gz-out`: after pfh_reads_gz_out(1) the next pfh_trim_fastq, pfh_trim_fastq_pair, pfh_mask_fastq or pfh_mask_fastq_counted of this
 * thread writes every read output as blocked gzip, deflated on the device (K-DEFLATE); the call takes the switch back. */
void pfh_reads_gz_out(int on);
int pfh_inflate_parse_member(const uint8_t *bytes, uint64_t n, uint32_t fields[4]);
int pfh_inflate_member(const uint8_t *payload, uint32_t n_in, uint8_t *out, uint32_t isize, uint32_t *produced, uint32_t blocks[3]);
int pfh_inflate_bgzf_member(const uint8_t *bytes, uint64_t n, uint8_t *out, uint32_t *out_len, uint32_t blocks[3]);
uint32_t pfh_inflate_crc32(const uint8_t *bytes, uint64_t n);
uint32_t pfh_inflate_crc32_sliced(const uint8_t *bytes, uint32_t n, uint32_t n_lanes);
int pfh_inflate_file_clause(const uint8_t *first, uint64_t n_first, uint64_t file_size, int *clause);
const char *pfh_inflate_clause_text(int clause);

/* ---- blocked-gzip output (K-DEFLATE): the rule without a device (csrc/pf_deflate_rule.hpp) ----
 * pfh_deflate_member: text[0, n), n <= 65280 -> one BGZF member at out[0, return value); out_cap >= n + 31.  result = { the block's kind
 *   (0 stored, 1 fixed, 2 dynamic), literals, matches }.  -1: an argument out of these ranges.
 * pfh_deflate_bound: the bytes that hold any n_bytes of text cut into members of member_text: n_bytes + 31 a member. */
int64_t pfh_deflate_member(const uint8_t *text, uint32_t n, uint8_t *out, uint64_t out_cap, uint32_t result[3]);
uint64_t pfh_deflate_bound(uint64_t n_bytes, uint32_t member_text);

/* ---- FASTA (K-FASTA, `--fasta`): the rule without a device (csrc/pf_fasta_rule.hpp) ----
 * pfh_reads_fasta(1): the next pfh_count_fastq, pfh_build_fastq, pfh_build_colored_fastq, pfh_run_fastq or pfh_run_multi_fastq of this
 * thread reads every input (with pfh_reads_gz: every inflated input) whose first byte is '>' as FASTA; the call takes the switch back.
 * The trimmed forms of run refuse it by name (FASTA has no qualities to trim).
 * pfh_fasta_index: the host rule on one chunk -- the compacted text (text_out, text_cap bytes) and the table (read_off / read_len,
 * table_cap entries) of its whole records; *n_records / *n_bases are the sizes needed whatever the capacities.  0, or the clause
 * (pfh_fasta_clause_text): 1 = the text does not start with '>'. */
void pfh_reads_fasta(int on);
int pfh_fasta_index(const char *text, uint64_t n, int final, uint64_t *bytes_used, uint64_t *n_records, uint64_t *n_bases, char *text_out,
                    uint64_t text_cap, uint64_t *read_off, uint32_t *read_len, uint64_t table_cap);
const char *pfh_fasta_clause_text(int clause);

/* ---- plain gzip (K-GUNZIP, `--gz-plain`): the rule without a device (csrc/pf_gunzip_rule.hpp) ----
 * pfh_reads_gz(2) selects `--gz-plain` for the next reads call: an input with the gzip magic is blocked gzip (K-INFLATE, as with 1) or
 * any other gzip, inflated by K-GUNZIP.
 * pfh_gunzip_header: one member header at bytes[0, n): the clause, *len = its bytes.
 * pfh_gunzip_file_kind: what the first bytes of a file say with `--gz-plain`: 0 plain, 1 blocked gzip, 2 refused with *clause, 3 gzip.
 * pfh_gunzip_candidate: does a non-final dynamic block header start at `bit` of bytes[0, n)?  (the search of the find stage)
 * pfh_gunzip_call: one call of pf_inflate_gzip's algorithm on the host, lane 0 of 1: same arguments, same result; out_cap too small
 *   returns -1 with res->out_bytes = needed.  stats = the nine counters of pf_gunzip_stats.
 * pfh_gunzip_file: a whole file in memory through the loop the stream seams run (carry, trailer, next header), fed in blocks of
 *   block_bytes (0: at once): the clause (0: out[0, *out_len) holds the members' texts); *member (0-based) and *byte say where. */
int pfh_gunzip_header(const uint8_t *bytes, uint64_t n, uint64_t *len);
int pfh_gunzip_file_kind(const uint8_t *first, uint64_t n_first, uint64_t file_size, int *clause);
int pfh_gunzip_candidate(const uint8_t *bytes, uint64_t n, uint64_t bit);
int pfh_gunzip_call(const uint8_t *comp, uint64_t n_bytes, uint64_t start_bit, const uint8_t *window, uint32_t n_window, uint32_t piece_bytes,
                    uint8_t *out, uint64_t out_cap, uint8_t *new_window, pf_gunzip_result *res, uint64_t stats[9]);
int pfh_gunzip_file(const uint8_t *bytes, uint64_t n, uint32_t piece_bytes, uint64_t block_bytes, uint64_t carry_max, uint8_t *out, uint64_t out_cap,
                    uint64_t *out_len, uint64_t *member, uint64_t *byte, uint64_t stats[9]);
const char *pfh_gunzip_clause_text(int clause);

/* ---- heterozygous k-mer pairs: `ploidyfrost smudge` and `run --smudge` (K-HETPAIR, pf_hetpairs in ploidyfrost_hip.h) ----
 * The rule, the summary and the text of the report: csrc/pf_hetpair_rule.hpp (PARITY UNPINNED: Smudgeplot is not part of the build).
 * pfh_hetpairs_host: the host's plain restatement, no device -- distinct canonical keys and their counters in, table (W * W cells,
 * W = hi - lo + 1, may be null), the pairs in the order of x (at most cap of *n_pairs are copied; the arrays may be null) and the
 * statistics out; returns 0, the rule's refusal (lo < 1, lo > hi, W > 4096, k) or -1 for a missing argument.  pfh_smudge_report_text:
 * table, statistics and n (0: none) to the report; *len = the bytes of the text, of which at most cap go to out.  pfh_smudge_of: the
 * smudge (p, m) of a pair with the coverages a <= b at the haploid coverage n.  pfh_smudge: the sub-command -- db_prefix, or inputs
 * counted with k, ci, cx, cs (db_prefix null; takes the pfh_reads_gz / pfh_reads_fasta switches); the bounds lo and hi or auto_cutoffs
 * (lo = `cutoffL -d`, hi = `cutoffU -d [quantile]` of the counters); n_hap (0: no summary); pairs_path (null: none).  It writes
 * <out>_smudge.tsv under a temporary name, renamed at the end; 0 = ok, else pfh_last_error(NULL) words the refusal and nothing is left
 * under an output name. */
typedef struct pfh_smudge_result {
    pf_hetpair_stats stats;
    uint32_t k, lo, hi, clamped;        /* the bounds that were used; clamped: hi was lowered to lo + 4095 */
    uint32_t proposed_p, proposed_m;    /* with n_hap: the label with the most pairs (0, 0: no pair) */
    uint64_t proposed_pairs, all_pairs;
} pfh_smudge_result;
/* `run --smudge [--smudge-n N] [--smudge-pairs FILE]`: after pfh_reads_smudge(1, n_hap, pairs_path) the next pfh_run_fastq or
 * pfh_run_fastq_trimmed of this thread runs K-HETPAIR behind the table of its first pass (lo = L, hi = min(U, L + 4095)) and writes
 * PloidyFrost_output/<out_prefix>_smudge.tsv, every other output being what it is without; n_hap < 0: no haploid coverage,
 * pairs_path null: no pairs file.  The call takes the switch back; pfh_reads_smudge_result gives what it found.  pfh_run_multi_fastq*
 * refuse the switch as not built. */
void pfh_reads_smudge(int on, int64_t n_hap, const char *pairs_path);
void pfh_reads_smudge_result(pfh_smudge_result *out);
int pfh_hetpairs_host(const uint64_t *kmers, const uint32_t *counts, uint64_t n, uint32_t k, uint32_t lo, uint32_t hi, uint64_t *table, uint64_t *pair_x,
                      uint64_t *pair_y, uint32_t *cov_x, uint32_t *cov_y, uint64_t cap, uint64_t *n_pairs, pf_hetpair_stats *stats);
int pfh_smudge_report_text(const uint64_t *table, const pf_hetpair_stats *stats, uint32_t k, uint32_t lo, uint32_t hi, uint64_t n, char *out, uint64_t cap,
                           uint64_t *len);
int pfh_smudge_of(uint64_t a, uint64_t b, uint64_t n, uint32_t *p, uint32_t *m);
int pfh_smudge(const char *db_prefix, const char *const *inputs, uint32_t n_inputs, uint32_t k, uint64_t ci, uint64_t cx, uint64_t cs, uint32_t lo, uint32_t hi,
               int auto_cutoffs, double quantile, uint64_t n_hap, const char *pairs_path, const char *out, uint64_t chunk_bytes, uint64_t initial_slots,
               int device, pfh_smudge_result *result);

/* Kmer::hash(seed) of the reference's Bifrost build (wyhash over the 8-byte left-aligned k-mer) */
uint64_t pfh_bifrost_kmer_hash(uint64_t left_aligned_kmer, uint64_t seed);

#ifdef __cplusplus
}
#endif
#endif
