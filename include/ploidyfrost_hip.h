/*
 * ploidyfrost_hip.h -- C ABI of the MI355X (gfx950) device layer for PloidyFrost's
 * superbubble + variant-calling hot path.
 *
 * PloidyFrost has no plugin/FFI mechanism: its hot path sits behind the C++ classes CDBG
 * (reference src/CDBG.hpp:20-41) and CCDBG, called only from main() (src/Main.cpp:829-849).
 * This header is the boundary a maintainer would bind instead: every entry point names the
 * reference function(s) whose compute it replaces.  Plain C types only; every buffer is
 * caller-allocated; every call returns an int status (PF_OK = 0) instead of exit();
 * one context per host thread / per GPU.
 *
 * Pointers marked [host|dev] may be host or device addresses (copied with
 * hipMemcpyDefault), which lets a PyTorch caller hand in tensor storage directly.
 *
 * Conventions
 *   unitig index u : 0-based, in the reference's iteration order (id = u + 1,
 *                    src/CDBG.cpp:131-136: long unitigs in S-line order, then short ones)
 *   oriented vertex: ov = 2*u + (strand ? 0 : 1); ov ^ 1 is the reverse complement
 *   k-mer          : uint64, 2 bits/base (A0 C1 G2 T3), first base most significant,
 *                    right aligned; 3 <= k <= 31
 *   PF_NONE        : empty adjacency slot / no vertex
 */
#ifndef PLOIDYFROST_HIP_H_
#define PLOIDYFROST_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PF_NONE 0xFFFFFFFFu

enum pf_status {
    PF_OK = 0,
    PF_ERR_ARG = 1,         /* bad argument / call order */
    PF_ERR_HIP = 2,         /* HIP runtime error, see pf_last_error() */
    PF_ERR_NO_DEVICE = 3,   /* no gfx950 device visible: there is no CPU fallback */
    PF_ERR_OVERFLOW = 4,    /* a caller-provided output buffer is too small */
    PF_ERR_MISSING_KMER = 5 /* a graph k-mer is absent from the count table
                               (the reference exit()s: src/CDBG.cpp:52-56, 92-96) */
};

typedef struct pf_ctx pf_ctx;

/* ---- context ------------------------------------------------------------------------- */
int pf_create(int device, pf_ctx **out);
/* Optional: initialise the HIP runtime and the device ahead of pf_create, e.g. on a helper thread while input files are read. */
int pf_warmup(int device);
void pf_destroy(pf_ctx *);
const char *pf_last_error(const pf_ctx *); /* ctx may be NULL: last creation error */
/* Launch on this hipStream_t (e.g. torch's current stream) instead of the context's own. */
int pf_set_stream(pf_ctx *, void *hip_stream);
int pf_synchronize(pf_ctx *);
/* Per-kernel HIP-event timing: when enabled every launch is bracketed by events on the
 * launch stream; pf_kernel_time() synchronises and returns the accumulated time / count. */
enum pf_kernel {
    PF_K_TABLE_BUILD = 0, PF_K_ADJ_INSERT, PF_K_ADJ_PROBE, PF_K_COV, PF_K_BFS, PF_K_BFS_BIG,
    PF_K_ALIGN, PF_K_ALIGN_BIG, PF_K_STRCOV, PF_K_BUBBLE, PF_K_BUBBLE_BIG, PF_K_COV_COLORED, PF_K_STRCOV_COLORED, PF_K_GMM, PF_K_KMC_DECODE, PF_K_MINZ, PF_K_COV_JOIN,
    PF_K_CALL_SCAN, PF_K_CALL_PREP, PF_K_CALL_PATHS, PF_K_CALL_SITES, PF_K_CALL_FORMAT, PF_K_CALL_SNP, PF_K_BFS_THREAD, PF_K_CALL_PAIR, PF_K_CALL_STACK,
    PF_K_COV_JOIN_REST, /* second kernel of K-COV-JOIN: the look-ups whose first line was full */
    PF_K_COPY_TEXT, /* not a kernel of this library: the copies of result text to the host (the runtime moves them with a kernel of its own) */
    PF_K_CALL_MODEL, /* the kernels of one pf_call_model_take (rows of a piece's text -> the model's values), timed as one launch */
    PF_K_DENSITY, /* the kernels of one pf_gmm_density, timed as one launch; unit: values x grid points */
    PF_K_HIST, /* K-HIST (pf_count_histogram); unit: counters */
    PF_K_MASK, /* K-MASK: everything one pf_mask_reads / pf_mask_fastq launches (index, classes, flag, paint), timed as one launch; unit: windows */
    PF_K_COUNT, /* K-COUNT: everything one pf_count_reads / pf_count_fastq launches (index, classes, insert, growth), timed as one launch; unit: windows */
    PF_K_TRIM, /* K-TRIM: everything one pf_trim_fastq / pf_trim_fastq_pair launches (index, intervals, sizes, scan, copy), timed as one launch; unit: records */
    PF_K_UNITIG, /* K-UNITIG: everything one pf_unitig_build launches (index, adjacency, link, simplify, rank, cycles, emit), timed as one launch; unit: k-mers */
    PF_K_MASKCOUNT, /* K-MASKCOUNT: everything one pf_maskcount_reads / pf_maskcount_fastq launches (index, classes, flag, insert, growth), timed as one launch; unit: windows */
    PF_K_UNION, /* K-UNION: everything one pf_kmer_union launches (check, the count and write kernels of every merge, their scans), timed as one launch; unit: keys given */
    PF_K_COLORSET, /* K-COLORSET: the kernel of one pf_color_kmers; unit: keys */
    PF_K_TRIMCOUNT, /* K-TRIMCOUNT: everything one pf_trim_table_fastq* / pf_count_fastq*_trimmed / pf_maskcount_fastq*_trimmed launches (index, intervals, table, then K-COUNT's or K-MASKCOUNT's core), timed as one launch; unit: records */
    PF_K_INFLATE, /* K-INFLATE: everything one pf_inflate_bgzf launches (headers, scan, inflate with the CRC), timed as one launch; unit: inflated bytes */
    PF_K_GUNZIP, /* K-GUNZIP: everything one pf_inflate_gzip launches (find, count, chain, decode, window, resolve with the CRC), timed as one launch; unit: inflated bytes */
    PF_K_FASTA, /* K-FASTA: everything the index of one pf_fasta_index / pf_count_fasta / pf_maskcount_fasta / pf_color_fasta call launches (newlines, lines, words, scans, compact, table), timed as one launch; the core behind it is timed under its own kernel; unit: bytes of the chunk */
    PF_K_DEFLATE, /* K-DEFLATE: everything one pf_deflate_bgzf launches (deflate, scan of the members' sizes, pack), timed as one launch; unit: bytes of text */
    PF_K_CLIP, /* K-CLIP: the kernels one pf_trim_fastq* / pf_trim_table_fastq* / pf_*_fastq*_trimmed call launches to clip adapters while a clip is open (one per file), timed as one launch inside the call's own; unit: records */ PF_K_PALIN, /* K-PALIN: the kernel one pf_trim_fastq_pair / pf_trim_table_fastq_pair / pf_*_fastq_pair_trimmed call launches behind K-CLIP's while a clip with prefix pairs is open (palindrome mode), timed as one launch inside the call's own; unit: pairs */ PF_K_QC, /* K-QC: the kernel one pf_qc_fastq call, or one pf_trim_fastq* / pf_trim_table_fastq* / pf_*_fastq*_trimmed call while a report is open, launches per file to add its records to the report's tables, timed as one launch per file inside the call's own; unit: records */ PF_K_HETPAIR, /* K-HETPAIR: everything one pf_hetpairs launches (flag, scan, write, table), timed as one launch; unit: keys in range */ PF_K_DEDUP, /* K-DEDUP: the kernels one pf_trim_fastq* / pf_trim_table_fastq* / pf_*_fastq*_trimmed call launches while a dedup is open, or one pf_dedup_keys call (growth, insert, verdict), timed as one launch inside the call's own; unit: units that take part */
    PF_K_COUNT_
};
int pf_enable_timing(pf_ctx *, int on);
int pf_kernel_time(pf_ctx *, int kernel, double *total_ms, uint64_t *launches);
int pf_reset_timing(pf_ctx *);
/* Which kernels pf_enable_timing times: bit k of the mask = launches of kernel k (default: all).  Two events per launch are not
 * free on a pass of a hundred launches from four host threads; a caller that wants one kernel's durations inside a region it
 * also times as a whole (bench.py: K-BUBBLE for the roofline) selects that kernel alone. */
int pf_timing_select(pf_ctx *, uint64_t kernel_mask);
/* The union of the timed launches' intervals of the kernels of the mask, in ms: what a kernel that is launched several times side by
 * side (K-BUBBLE: a launch per size class and align range) really occupies of a pass -- the sum pf_kernel_time gives counts the
 * overlap as often as there are launches. */
int pf_kernel_busy(pf_ctx *, uint64_t kernel_mask, double *busy_ms);
/* Device-busy time of everything timed since the last reset: the UNION of the launches' [start, end] intervals (HIP events on the
 * streams they were launched on), in ms -- the launches of the calling pipeline overlap (two align ranges, K-BUBBLE's classes on
 * streams of their own, K-TEXT beside the next range's alignment), so the sum pf_kernel_time gives counts overlapped time twice;
 * *span_ms = first start to last end.  Library launches between them (rocPRIM scans / sorts, copies, fills) are not timed. */
int pf_device_busy(pf_ctx *, double *busy_ms, double *span_ms);
/* Work items the timed launches of a kernel were given since the last reset, in the unit its algorithmic bytes are quoted per
 * (DESIGN.md 3): candidates for K-BFS's tiers, bubbles for K-SNP / K-PAIR / K-BUBBLE / K-PATHS / K-SITES / K-TEXT, sides for K-SCAN. */
int pf_kernel_units(pf_ctx *, int kernel, uint64_t *units);
const char *pf_kernel_name(int kernel);

/* ---- graph (replaces Bifrost's CompactedDBG storage for this path) --------------------- */
/* Packed unitigs: unitig u occupies words [seq_off[u], seq_off[u] + ceil(len_bp[u]/32)) of
 * seq_words; base j sits in word j/32 at bits [62 - 2*(j%32), 63 - 2*(j%32)] (first base
 * most significant), padding bits zero.  seq_off has n_unitigs + 1 entries. [host|dev] */
int pf_upload_graph(pf_ctx *, const uint64_t *seq_words, const uint64_t *seq_off, const uint32_t *len_bp,
                    uint32_t n_unitigs, int k);
/* K-GFA (pf_gfa.hip): the same graph straight from the bytes of a Bifrost GFA file -- the parse half of CompactedDBG::read
 * (bifrost/src/CompactedDBG.tcc:823-960, 7888-7908; GFA_Parser.cpp:380-520) on the device.  body = the file after its header
 * line [host|dev], gfa_version 1 or 2 (the header's VN:Z), k from its KL:Z.  Segment lines are located, their sequences packed two
 * bits per base, the k-length ones canonicalised; the graph is resident afterwards as after pf_upload_graph, in the unitig order
 * of pf_upload_graph's callers before abundant k-mers are moved (segments longer than k in file order, then the k-length ones).
 * PF_ERR_ARG with the loader's messages: "missing fields in a segment line", "segment shorter than k", "non-ACGT base in a
 * segment", "no segments in the GFA file".  A sequence field is every byte between its tabs / the line feed, as GFA_Parser.cpp:497-520
 * takes it: the '\r' that ends the sequence of a CRLF file is its last base (A in a segment longer than k, CompressedSequence.cpp:597-614;
 * T in a k-length one, Kmer.cpp:92-107), as in the reference; any other byte that is no base is refused.  pf_gfa_segments hands the host what it keeps per unitig (once per ingest; any
 * pointer may be NULL): length, offset of the sequence field inside body, file rank among the segments, the DA:Z tag (-1 =
 * none; *any_da = some segment had one), and whether a k-length unitig is stored as its reverse complement. */
int pf_gfa_ingest(pf_ctx *, const char *body, uint64_t n_bytes, int gfa_version, int k, uint32_t *n_unitigs, uint32_t *n_short);
/* The same in two steps: pf_gfa_parse (locate + pack, on a stream of its own, touching nothing else of the context: it may run
 * on one thread while another feeds the count table to the same context; its error text: pf_gfa_error) and pf_gfa_upload (the
 * packed arrays become the context's graph, as pf_upload_graph). */
int pf_gfa_parse(pf_ctx *, const char *body, uint64_t n_bytes, int gfa_version, int k, uint32_t *n_unitigs, uint32_t *n_short);
int pf_gfa_upload(pf_ctx *);
const char *pf_gfa_error(const pf_ctx *);
int pf_gfa_segments(pf_ctx *, uint32_t *len_bp, uint64_t *seq_off, uint32_t *file_rank, int16_t *da_tag, uint8_t *stored_rc, int *any_da);
/* G2: neighbour discovery (bifrost/src/NeighborIterator.tcc:25-47 via
 * CompactedDBG::find(km, extremities_only=true), CompactedDBG.tcc:1403-1523): joins the
 * end k-mers of all unitigs on the device and fills the CSR kept in the context.
 * succ/pred (2*n_unitigs*4 entries, A,C,G,T slot order) may be NULL. [host|dev] */
int pf_build_adjacency(pf_ctx *, uint32_t *succ, uint32_t *pred);

/* ---- k-mer count table (replaces CKMCFile, KMC/kmc_api/kmc_file.cpp) ------------------- */
/* K-MINZ (GFA ingest, unitig numbering): how often does the most frequent minimizer occur in the uploaded graph?  Bifrost numbers
 * a k-length unitig last when the bucket of its minimizer already holds 15 entries (CompactedDBG.tcc:3928-4080); the loader has to
 * replay that bookkeeping on the host only when some bucket can get that full.  Counts every g-mer position that is the minimum
 * (bifrost/src/RepHash.hpp hash; not at either end of the k-mer, minHashIterator.hpp:63-119) of the window of some k-mer containing it,
 * in a table of pf_minimizer_table_slots(n_kmers) slots indexed by a mix of the canonical minimizer -- per slot an upper bound of
 * the entries Bifrost can file there.  *max_occurrences < 15  =>  no abundant k-mer: ids are long unitigs, then k-length ones, in
 * file order.  crowded_slots (optional): slots that reached `limit`; table_out (optional, host or device): the u32 counters. */
uint64_t pf_minimizer_table_slots(uint64_t n_kmers);
int pf_minimizer_crowding(pf_ctx *, int g, uint32_t limit, uint32_t *max_occurrences, uint64_t *crowded_slots, uint32_t *table_out);
/* For a graph that CAN crowd a bucket (max_occurrences >= limit), what the host replay of Bifrost's bookkeeping
 * (csrc/host/pf_host_minz.cpp) otherwise computes in two passes of its own over every unitig: the census table narrowed to
 * saturating bytes (pf_minimizer_table_slots(n_kmers) of them) and, per unitig in upload order, whether one of its counted positions
 * falls into a slot that reached `limit` -- the unitigs that have to go through addUnitig's replay.  Both are upper bounds of the
 * host's own (ties inside a window count twice here), which only makes the replay follow a few more buckets and unitigs.
 * counters8_out, unitig_flags_out: [host|dev] */
int pf_minimizer_replay_inputs(pf_ctx *, int g, uint32_t limit, uint8_t *counters8_out, uint8_t *unitig_flags_out);

/* K-KMC: KMC database ingest on the device.  `records` = the record area of <db>.kmc_suf (after its 4-byte marker): n_records
 * records of suffix_bytes = (k - lut_prefix_len) / 4 suffix bytes (most significant first) + counter_bytes counter bytes (least
 * significant first), ordered as the prefix table says (KMC/kmc_api/kmc_file.cpp:185-302, 775-782): lut[e] = index of the first
 * record of table entry e, e = prefix for the KMC1 layout and bin * 4^p + prefix for the KMC2 (signature-binned) layout, with
 * n_lut entries plus lut[n_lut] = n_records.  Output: two device arrays (exact k-mers as stored, counts truncated to 32 bits)
 * to hand to pf_upload_counts / pf_upload_counts_colored, released with pf_device_free.  records: [host|dev]; lut: host */
int pf_kmc_decode(pf_ctx *, const uint8_t *records, uint64_t n_records, uint32_t suffix_bytes, uint32_t counter_bytes,
                  const uint64_t *lut, uint64_t n_lut, uint32_t lut_prefix_len, uint32_t k, uint64_t **kmers_dev, uint32_t **counts_dev);
void pf_device_free(pf_ctx *, void *device_pointer);
/* K-HIST: the k-mer histogram of a database from the counters pf_kmc_decode left on the device -- the file the reference's
 * cutoffL / cutoffU / -h read (src/Main.cpp:200-277) and step 1 of its workflow makes with a second tool and a second pass over the
 * database (`kmc_tools transform <db> histogram <file>`).  For every counts[i] with lo <= counts[i] <= hi:
 * hist[min(counts[i], n_bins - 1)] += 1; every other bin is 0 (n = 0 or lo > hi: all of them).  Integers only: the same bits on
 * every call.  n_bins from 1 to PF_HIST_MAX_BINS, else PF_ERR_ARG.  counts, hist: [host|dev] */
#define PF_HIST_MAX_BINS (1u << 20)
int pf_count_histogram(pf_ctx *, const uint32_t *counts, uint64_t n, uint64_t lo, uint64_t hi, uint32_t n_bins, uint64_t *hist);
/* K-MASK: low-coverage k-mers of reads masked against the count table (pf_upload_counts comes first) -- what step 2 of the
 * reference's workflow does with `kmc_tools filter -hm <db> <reads> -ci<L>`, whose inner loop is CKMCFile::GetCountersForRead
 * (KMC/kmc_api/kmc_file.cpp:904-1090).  The rule (csrc/pf_mask_rule.hpp): a read s[0..n) has one window per i in 0 .. n - k, k the
 * table's k-mer length; its counter is 0 when the window holds a byte outside ACGTacgt, else the count the table holds for it (lower
 * case read as upper case; a both_strands table is asked for the canonical form, any other for the window as it reads; absent, or
 * outside the header's [min_count, max_count]: 0).  A window is bad when its counter is below low or above up (up = 0xFFFFFFFF: no
 * upper bound).  A byte of a read becomes 'N' when a bad window covers it; every other byte of the text is copied.  PARITY with
 * kmc_tools UNPINNED (the tool is not part of the build): the other reading would mask only bases that no good window covers.
 * Integer sums: the same bytes and statistics on every call.  Without a table: PF_ERR_ARG, by name. */
typedef struct pf_mask_stats {
    uint64_t reads;          /* records seen */
    uint64_t reads_changed;  /* records in which at least one byte changed */
    uint64_t bases;          /* sequence bytes */
    uint64_t bases_masked;   /* bytes that changed to N (an input N under a bad window does not count) */
    uint64_t kmers;          /* windows */
    uint64_t kmers_bad;      /* bad windows */
} pf_mask_stats;
/* reads given explicitly: read i = text[read_off[i] .. read_off[i] + read_len[i]), ascending and without overlaps (else PF_ERR_ARG
 * with the first offender); out = text with the rule applied.  text, read_off, read_len, out: [host|dev]; out may not alias text.
 * n_reads = 0 or n_bytes = 0 is not an error. */
int pf_mask_reads(pf_ctx *, const char *text, uint64_t n_bytes, const uint64_t *read_off, const uint32_t *read_len,
                  uint64_t n_reads, uint32_t low, uint32_t up, char *out, pf_mask_stats *stats);
/* one chunk (fewer than 2^32 bytes) of a FASTQ file with four lines per record: index, check, mask.  Lines end in '\n'; a '\r'
 * directly before it belongs to the line end; roles come from the line's index.  final = 0: the chunk may end inside a record;
 * *bytes_used is the end of the last whole record, out is written up to there, and the caller carries the rest into the next chunk.
 * final = 1: the last line may lack its '\n'.  On a format error (first line without '@', third without '+', quality and sequence of
 * different lengths, with final a line count that is no multiple of four): PF_ERR_ARG, *bad_record is the 0-based record within the
 * chunk (the smallest offender), pf_last_error names the clause, and nothing has been written to out.  text, out: [host|dev] */
int pf_mask_fastq(pf_ctx *, const char *text, uint64_t n_bytes, int final, uint32_t low, uint32_t up, char *out,
                  uint64_t *bytes_used, pf_mask_stats *stats, uint64_t *bad_record);
/* K-COUNT: k-mers counted from reads on the device -- what step `2.kmc_db` of the reference's workflow does with
 * `kmc -k<k> -ci<ci> -cs<cs> -cx<cx> [-b]`.  The rule (csrc/pf_count_rule.hpp): the windows are K-MASK's (one per i in 0 .. n - k of a
 * read, counted when all k bytes are in ACGTacgt, lower case read as upper case); the key is the canonical form min(fw, rc), or with
 * both_strands = 0 the window as it reads; a counter is the exact number of counted windows of its key over all calls, a uint32 that
 * never wraps (PF_ERR_OVERFLOW, "a k-mer occurs more than 4294967295 times").  A k-mer is given out when ci <= c <= cx, with the value
 * min(c, cs).  The table lies in HBM and grows by itself; when it cannot (free memory), PF_ERR_OVERFLOW by name with the number of
 * distinct k-mers reached.  PARITY with kmc UNPINNED (the tool is not part of the build).  Integer sums: the same arrays on every run,
 * whatever the chunking. */
typedef struct pf_count_stats {
    uint64_t reads;      /* records seen */
    uint64_t bases;      /* sequence bytes */
    uint64_t kmers;      /* windows */
    uint64_t kmers_bad;  /* windows holding a byte outside ACGTacgt: not counted */
    uint64_t unique;     /* pf_count_finish only: distinct k-mers counted */
    uint64_t below_min;  /* ... of them with c < ci */
    uint64_t above_max;  /* ... with c > cx */
    uint64_t written;    /* ... given out */
} pf_count_stats;
/* opens a count: 3 <= k <= 31.  initial_slots = 0: twice the first call's bytes; else rounded up to a power of two of at least 64.
 * A second begin without pf_count_finish / pf_count_abort: PF_ERR_ARG by name. */
int pf_count_begin(pf_ctx *, uint32_t k, int both_strands, uint64_t initial_slots);
/* reads given explicitly, as pf_mask_reads takes them (ascending, no overlaps, else PF_ERR_ARG with the first offender); stats: this
 * call's reads, bases, kmers, kmers_bad.  text, read_off, read_len: [host|dev] */
int pf_count_reads(pf_ctx *, const char *text, uint64_t n_bytes, const uint64_t *read_off, const uint32_t *read_len, uint64_t n_reads,
                   pf_count_stats *stats);
/* one chunk of a FASTQ file: the chunk contract and the format clauses of pf_mask_fastq; nothing is counted from a refused chunk.
 * text: [host|dev] */
int pf_count_fastq(pf_ctx *, const char *text, uint64_t n_bytes, int final, uint64_t *bytes_used, pf_count_stats *stats, uint64_t *bad_record);
/* closes the count: the k-mers with ci <= c <= cx, sorted, and min(c, cs), as two device arrays like pf_kmc_decode's (for
 * pf_count_histogram, pf_upload_counts, pf_kmc_encode; released with pf_device_free); stats: the totals of all calls and the four
 * finish fields.  ci < 1, ci > cx, cs < 1 or a value above 2^32 - 1: PF_ERR_ARG by name, and the count stays open. */
int pf_count_finish(pf_ctx *, uint64_t ci, uint64_t cx, uint64_t cs, uint64_t **kmers_dev, uint32_t **counts_dev, uint64_t *n, pf_count_stats *stats);
int pf_count_abort(pf_ctx *);
/* K-MASKCOUNT: `mask` followed by the count of `build` in one pass and without the masked text -- every window of the reads that
 * would still hold k bytes of ACGTacgt after K-MASK had painted its Ns is counted into the open count.  The rule
 * (csrc/pf_run_rule.hpp): with bad(q) as K-MASK defines it against the resident table (window q's counter outside [low, up]) and
 * valid(p) as K-COUNT does (all k bytes are bases), window p counts when valid(p) and no q in [p - k + 1, p + k - 1] is bad; the key
 * is the canonical form.  Both calls need a resident count table (pf_upload_counts) and an open count (pf_count_begin, both strands)
 * whose k equals the table's: each missing piece is PF_ERR_ARG by name.  They add to the open count as pf_count_reads /
 * pf_count_fastq do -- the same growth and the same refusals -- and pf_count_finish closes it: the same arrays whatever the chunking,
 * equal to those of pf_mask_* followed by pf_count_* on the masked text. */
typedef struct pf_maskcount_stats {
    uint64_t reads;          /* records seen */
    uint64_t bases;          /* sequence bytes */
    uint64_t kmers;          /* windows */
    uint64_t kmers_invalid;  /* windows holding a byte outside ACGTacgt */
    uint64_t kmers_bad;      /* bad windows (pf_mask_stats::kmers_bad) */
    uint64_t kmers_kept;     /* windows counted */
} pf_maskcount_stats;
/* reads given explicitly, as pf_mask_reads takes them.  text, read_off, read_len: [host|dev] */
int pf_maskcount_reads(pf_ctx *, const char *text, uint64_t n_bytes, const uint64_t *read_off, const uint32_t *read_len, uint64_t n_reads,
                       uint32_t low, uint32_t up, pf_maskcount_stats *stats);
/* one chunk of a FASTQ file: the chunk contract and the format clauses of pf_mask_fastq; nothing is counted from a refused chunk.
 * text: [host|dev] */
int pf_maskcount_fastq(pf_ctx *, const char *text, uint64_t n_bytes, int final, uint32_t low, uint32_t up, uint64_t *bytes_used,
                       pf_maskcount_stats *stats, uint64_t *bad_record);
/* the inverse of K-KMC: sorted distinct k-mers and their counts as the record area of a KMC1 <db>.kmc_suf (n records of
 * (k - lut_prefix_len) / 4 suffix bytes, most significant first, + counter_bytes counter bytes, least significant first) and the
 * prefix table of its <db>.kmc_pre (4^lut_prefix_len entries plus lut[4^lut_prefix_len] = n).  Either output may be NULL (a block of
 * records needs no table).  kmers, counts, records_out, lut_out: [host|dev] */
int pf_kmc_encode(pf_ctx *, const uint64_t *kmers, const uint32_t *counts, uint64_t n, uint32_t k, uint32_t lut_prefix_len, uint32_t counter_bytes,
                  uint8_t *records_out, uint64_t *lut_out);
/* K-UNITIG: the compacted de Bruijn graph of reads built on the device -- what step `4.bifrost` of the reference's workflow does with
 * `Bifrost build [-i] [-d] -k <k> -r reads.fq -o sample`.  The rule (csrc/pf_unitig_rule.hpp): the vertices are the sorted distinct
 * canonical k-mers pf_count_finish gives (ci = 1); an oriented k-mer x links to y when succ(x) == [y], pred(y) == [x] and they are
 * different k-mers, a unitig is a maximal chain of links; with clip_tips (-i) and / or del_isolated (-d) the unitigs of fewer than k
 * k-mers that CompactedDBG::removeUnitigs removes go, and what is left is compacted once more.  The text of <sample>.gfa stays on the
 * device until pf_unitig_release: the H line (KL = k, ML = g), then one `S <id> <sequence>` line per unitig, each in the reading
 * whose first k-mer is the smaller one (a closed cycle from its smallest canonical k-mer), ascending by that k-mer, ids from 1, no L
 * lines.  The same bytes on every call.  Single-sample graphs only. */
#define PF_UNITIG_STAGES 6 /* index, adjacency + link, simplify, rank, cycles, emit */
typedef struct pf_unitig_stats {
    uint64_t distinct;     /* k-mers given */
    uint64_t unitigs;      /* unitigs before simplifying */
    uint64_t removed;      /* of them removed by clip_tips / del_isolated */
    uint64_t unitigs_out;  /* S lines */
    uint64_t longest;      /* bases of the longest sequence */
    uint64_t bytes;        /* of the text, header line included */
    uint64_t cycles;       /* closed cycles among the S lines */
    uint64_t rounds;       /* pointer-jumping rounds of the rank stage (at most ceil(log2(2 n)) + 1) */
    uint64_t cycle_rounds; /* the same of the cycle stage (0 without a closed cycle) */
    double stage_ms[PF_UNITIG_STAGES]; /* device time of each stage, from events on the launch stream */
} pf_unitig_stats;
/* kmers: n sorted distinct canonical k-mers of length k, [host|dev] (anything else: PF_ERR_ARG by name); 3 <= k <= 31, 1 <= g <= k - 2 or
 * g = PF_UNITIG_G_DEFAULT (Bifrost's default for k: k - 8 from k = 15, k - 4 from k = 7, else k - 2),
 * n < 2^31, else PF_ERR_ARG.  Buffers that do not fit the free device memory: PF_ERR_OVERFLOW by name with n.  A second build without
 * pf_unitig_release: PF_ERR_ARG by name. */
#define PF_UNITIG_G_DEFAULT 0xFFFFFFFFu
int pf_unitig_build(pf_ctx *, const uint64_t *kmers, uint64_t n, uint32_t k, uint32_t g, int clip_tips, int del_isolated, pf_unitig_stats *stats);
/* bytes [first_byte, first_byte + len) of the text to the host; outside the text, or without a build: PF_ERR_ARG */
int pf_unitig_fetch(pf_ctx *, uint64_t first_byte, uint64_t len, char *host);
/* the resident text itself, for a reader on the same device (pf_gfa_parse takes the bytes behind the header line as its body):
 * *text_dev [dev], *n_bytes as pf_unitig_stats::bytes; valid until pf_unitig_release.  Without a build: PF_ERR_ARG by name. */
int pf_unitig_text(pf_ctx *, const char **text_dev, uint64_t *n_bytes);
int pf_unitig_release(pf_ctx *);
/* K-COLOR: the coloured graph of several files of reads -- what `Bifrost build -c -r s0.fq -r s1.fq ...` writes beside the graph.  The
 * rule: csrc/pf_color_rule.hpp.  pf_unitig_build_colored is pf_unitig_build on the k-mers of all files together (same graph, same line
 * order and ids) that also places every line's colour set (n_seeds rounds, 1 .. 255; *overflow = lines left over), ends every S line in
 * `\tDA:Z:<round>` (0: overflow table) and keeps every live k-mer's place in graph order in the context.  pf_color_begin(n_colors, 1 ..
 * 1024) builds the look-up table over those k-mers and clears one bit plane per colour (what does not fit: PF_ERR_OVERFLOW by name with
 * the counts; a unitig with n_colors * k-mers >= 2^32: PF_ERR_ARG by name).  pf_color_reads / pf_color_fastq stream the reads of colour
 * `colour` as pf_count_reads / pf_count_fastq take them (stats: that call's).  pf_color_finish turns the planes into runs of ids
 * colour * m + position per line (stats: the whole colouring's); pf_color_fetch copies per line the head k-mer as written, the k-mer
 * count and the slot, run_off (lines + 1 entries) and the runs (two words each: first id, last id) to the host; any may be NULL.
 * pf_unitig_fetch gives the text, pf_unitig_release ends it all.  kmers: as pf_unitig_build; a device array stays the caller's and is
 * read until pf_color_begin has returned. */
typedef struct pf_color_stats {
    uint64_t colors;
    uint64_t reads;             /* records streamed */
    uint64_t windows_colored;   /* windows whose k-mer lies in the graph */
    uint64_t windows_unplaced;  /* windows of k bases whose k-mer -i / -d removed */
    uint64_t windows_bad;       /* windows that hold a byte outside ACGTacgt */
    uint64_t runs;
    uint64_t overflow;          /* lines placed by no round */
    uint64_t lines;
    uint64_t table_slots, plane_words;
    double table_ms, mark_ms, runs_ms; /* device time of the stages, from events on the launch stream */
} pf_color_stats;
int pf_unitig_build_colored(pf_ctx *, const uint64_t *kmers, uint64_t n, uint32_t k, uint32_t g, int clip_tips, int del_isolated, uint32_t n_seeds,
                            pf_unitig_stats *stats, uint64_t *overflow);
int pf_color_begin(pf_ctx *, uint32_t n_colors);
int pf_color_reads(pf_ctx *, uint32_t colour, const char *text, uint64_t n_bytes, const uint64_t *read_off, const uint32_t *read_len, uint64_t n_reads,
                   pf_color_stats *stats);
int pf_color_fastq(pf_ctx *, uint32_t colour, const char *text, uint64_t n_bytes, int final, uint64_t *bytes_used, pf_color_stats *stats,
                   uint64_t *bad_record);
/* K-FASTA: FASTA reads and assemblies -- one chunk of FASTA text turned on the device into what pf_count_reads, pf_maskcount_reads and
 * pf_color_reads take: the sequences of its whole records as one compacted text (one directly behind the other, no separator) and the
 * table (read_off, read_len) into it.  The rule (csrc/pf_fasta_rule.hpp): lines end at '\n', a '\r' directly in front of it is not
 * content; a line whose first byte is '>' is a header and opens a record; every other line is a sequence line of the record opened
 * last (an empty line: an empty one; a '>' elsewhere: a sequence byte; no byte is refused); reads = headers, bases = sequence bytes, a
 * record without a sequence byte is a read of length 0.  The chunk contract is pf_mask_fastq's with FASTA's meaning of "whole": with
 * final = 0 a record is whole when a later header line starts inside the chunk, and *bytes_used is the first byte of the last such
 * line (only one: no record, *bytes_used = 0, the caller carries everything); with final = 1 every record is whole.  A chunk starts at
 * a record start: a first byte other than '>' is PF_ERR_ARG ("record 0 of the chunk: ...").  n_bytes < 2^32 - 256.  No state crosses calls.
 * What a call makes of F is what its _fastq twin makes of Q(F) -- every record rewritten as "@header", the joined sequence, "+" and one
 * 'I' per base -- in counts, statistics and refusals of the core.
 * pf_fasta_index leaves the index on the device: *text_dev (*n_bases bytes, 16-byte aligned), *read_off_dev, *read_len_dev (*n_records
 * entries) belong to the context and are valid until its next K-FASTA call; pf_fasta_index_fetch copies them to the caller's buffers
 * (text_cap bytes, table_cap entries; too small: PF_ERR_ARG by name with the sizes needed, which n_records / n_bases then hold).
 * pf_count_fasta, pf_maskcount_fasta, pf_color_fasta: the contracts of pf_count_fastq, pf_maskcount_fastq, pf_color_fastq; each runs
 * K-FASTA and then pf_count_reads / pf_maskcount_reads / pf_color_reads over the compacted text on the device.  The index is timed as one
 * launch of PF_K_FASTA (unit: bytes of the chunk), the core as PF_K_COUNT / PF_K_MASKCOUNT.  text: [host|dev] */
#define PF_FASTA_TILE 4096 /* bytes of the chunk one block compacts at a time */
int pf_fasta_index(pf_ctx *, const char *text, uint64_t n_bytes, int final, uint64_t *bytes_used, uint64_t *n_records, uint64_t *n_bases,
                   const char **text_dev, const uint64_t **read_off_dev, const uint32_t **read_len_dev);
int pf_fasta_index_fetch(pf_ctx *, const char *text, uint64_t n_bytes, int final, uint64_t *bytes_used, uint64_t *n_records, uint64_t *n_bases,
                         char *text_out, uint64_t text_cap, uint64_t *read_off, uint32_t *read_len, uint64_t table_cap);
int pf_count_fasta(pf_ctx *, const char *text, uint64_t n_bytes, int final, uint64_t *bytes_used, pf_count_stats *stats, uint64_t *bad_record);
int pf_maskcount_fasta(pf_ctx *, const char *text, uint64_t n_bytes, int final, uint32_t low, uint32_t up, uint64_t *bytes_used,
                       pf_maskcount_stats *stats, uint64_t *bad_record);
int pf_color_fasta(pf_ctx *, uint32_t colour, const char *text, uint64_t n_bytes, int final, uint64_t *bytes_used, pf_color_stats *stats,
                   uint64_t *bad_record);
/* K-COLORSET: colour `colour` from the sorted or unsorted distinct canonical k-mers of its reads instead of from the reads (the rule:
 * csrc/pf_runmulti_rule.hpp) -- one look-up per key in the table pf_color_begin built, the same planes pf_color_reads sets from the
 * windows.  Between pf_color_begin and pf_color_finish; may be mixed with pf_color_reads / pf_color_fastq.  kmers_dev: [dev].  Refused by
 * name (PF_ERR_ARG): no colouring open, a colour of n_colors or more, an array that is not on the device. */
typedef struct pf_color_kmers_stats {
    uint64_t kmers;           /* keys given */
    uint64_t kmers_colored;   /* keys that lie in the graph */
    uint64_t kmers_unplaced;  /* keys the graph does not hold (-i / -d removed them, or they never were vertices) */
} pf_color_kmers_stats;
int pf_color_kmers(pf_ctx *, uint32_t colour, const uint64_t *kmers_dev, uint64_t n, pf_color_kmers_stats *stats);
int pf_color_finish(pf_ctx *, pf_color_stats *stats);
int pf_color_fetch(pf_ctx *, uint64_t *heads, uint32_t *m, uint32_t *slot, uint64_t *run_off, uint32_t *runs);
/* K-UNION: the sorted distinct union of n_sets (1 .. 1024) sorted distinct arrays of 64-bit keys on the device (csrc/pf_union.hip; the
 * rule: csrc/pf_runmulti_rule.hpp) -- the vertices of the coloured graph from the k-mers of every sample's masked reads.  sets_dev[c]:
 * [dev], n[c] keys (an empty set may be NULL); the inputs stay the caller's.  *out_dev: a fresh device array of *n_out keys, released with
 * pf_device_free; the same array on every call.  A set that is not on the device, not ascending or holds a key twice: PF_ERR_ARG by
 * name, before anything is merged.  What does not fit the free device memory: PF_ERR_OVERFLOW by name with the counts. */
int pf_kmer_union(pf_ctx *, uint32_t n_sets, const uint64_t *const *sets_dev, const uint64_t *n, uint64_t **out_dev, uint64_t *n_out);
/* K-TRIM: reads quality-trimmed on the device -- what step `1.trim` of the reference's workflow does with
 * `trimmomatic PE -phred33 ... LEADING:10 TRAILING:10 SLIDINGWINDOW:3:20 MINLEN:50`.  The rule (csrc/pf_trim_rule.hpp): the quality of
 * position i of a read of n bases is q[i] = (int)byte - phred (phred 33 or 64; signed); the state is an interval [b, e) of the read,
 * [0, n) at first, or dropped; up to PF_TRIM_MAX_STEPS steps apply in the order given.  LEADING:t  b = the first i of [b, e) with
 * q[i] >= t, none: dropped.  TRAILING:t  e = 1 + the last such i, none: dropped.  SLIDINGWINDOW:w:t  e - b < w: dropped; window j is
 * bad when q[b+j] + .. + q[b+j+w-1] < w * t; window 0 bad: dropped; else with j the first bad window e = b + j - 1 + w (the end of the
 * last good window).  MINLEN:l  e - b < l: dropped.  e == b after the last step: dropped.  0 <= t <= 93, 1 <= w <= 64.  A kept record is
 * written as header content, seq[b:e], plus-line content, qual[b:e], each followed by one '\n' (CRLF input comes out with '\n', a
 * last line without a newline gets one); a dropped record writes nothing.  PARITY with Trimmomatic UNPINNED (the tool is not part of
 * the build): whether bases below t at the end of the last good window go too is the one open point (pf_trim::sliding_end).
 * Integers only: the same bytes and statistics on every call.  Bad steps or a bad phred: PF_ERR_ARG by name. */
enum { PF_TRIM_LEADING = 1, PF_TRIM_TRAILING = 2, PF_TRIM_SLIDINGWINDOW = 3, PF_TRIM_MINLEN = 4 };
#define PF_TRIM_MAX_STEPS 8
typedef struct pf_trim_step {
    uint32_t kind;   /* PF_TRIM_LEADING .. PF_TRIM_MINLEN */
    uint32_t a;      /* t of LEADING / TRAILING, w of SLIDINGWINDOW, l of MINLEN */
    uint32_t b;      /* t of SLIDINGWINDOW, else 0 */
} pf_trim_step;
typedef struct pf_trim_stats {
    uint64_t reads;       /* per file: records seen */
    uint64_t kept;        /* ... written */
    uint64_t dropped;     /* ... not written */
    uint64_t bases;       /* ... quality bytes of the records seen */
    uint64_t bases_kept;  /* ... of them written */
    uint64_t both;        /* pair calls (else 0): pairs with both records kept */
    uint64_t only1;       /* ... with the record of file 1 alone */
    uint64_t only2;       /* ... with the record of file 2 alone */
    uint64_t neither;     /* ... with none */
} pf_trim_stats;
/* one chunk (fewer than 2^32 bytes) of a FASTQ file: the chunk contract and the format clauses of pf_mask_fastq; a refused chunk has
 * written nothing.  out holds n_bytes + 1 bytes, *out_bytes of them are written.  rec_begin / rec_len (may be NULL, one entry per
 * whole record of the chunk -- at most n_bytes / 4; len 0 = dropped).  text, out, rec_begin, rec_len: [host|dev] */
int pf_trim_fastq(pf_ctx *, const char *text, uint64_t n_bytes, int final, const pf_trim_step *steps, uint32_t n_steps, uint32_t phred,
                  char *out, uint64_t *out_bytes, uint64_t *bytes_used, uint32_t *rec_begin, uint32_t *rec_len, uint64_t *n_records,
                  pf_trim_stats *stats, uint64_t *bad_record);
/* one chunk of each file of a pair: record r of file 1 pairs with record r of file 2 (header names are not compared).  Both chunks are
 * indexed and n = the smaller of their whole-record counts is taken from each: bytes_used[f] = the end of record n - 1 of file f; final
 * chunks with different counts are refused by name.  Both kept: out[0] (o1) and out[2] (o2); file 1 alone: out[1] (u1); file 2 alone:
 * out[3] (u2); out[0], out[1] hold n1 + 1 bytes, out[2], out[3] n2 + 1.  *bad_record = 2 * record + file (0, 1).  stats[f]: file f;
 * the pair fields are the same in both.  The pointers inside out / rec_begin / rec_len: [host|dev] */
int pf_trim_fastq_pair(pf_ctx *, const char *text1, uint64_t n1, const char *text2, uint64_t n2, int final, const pf_trim_step *steps,
                       uint32_t n_steps, uint32_t phred, char *out[4], uint64_t out_bytes[4], uint64_t bytes_used[2], uint32_t *rec_begin[2],
                       uint32_t *rec_len[2], uint64_t *n_records, pf_trim_stats stats[2], uint64_t *bad_record);
/* K-TRIMCOUNT: K-TRIM folded into K-COUNT and K-MASKCOUNT -- one chunk of raw FASTQ (or one chunk of each file of a pair) trimmed and
 * counted in one call, without the trimmed text (the rule: csrc/pf_trimrun_rule.hpp).  The reads handed on are the sequence bytes
 * [seq_begin + b, seq_begin + e) of every whole record that K-TRIM keeps; for a pair, record r of a file is handed on only when record
 * r of BOTH files is kept (the reference counts trim1 / trim2, never the unpaired survivors).  They form a reads table as
 * pf_count_reads / pf_maskcount_reads take it, per file over that file's own text, and K-COUNT's / K-MASKCOUNT's rule applies to the
 * table unchanged: a window that reaches into the trimmed-off head or tail of a read is no window -- neither counted nor flagged bad.
 * The chunk contract, the format clauses and bad_record are pf_trim_fastq's / pf_trim_fastq_pair's (a refused chunk has counted
 * nothing); the step refusals are K-TRIM's; what the count calls need (an open count, a resident table, the same k, both strands,
 * low <= up) is what pf_count_fastq / pf_maskcount_fastq need.  All by name, under the entry point's name.  trim_stats: what
 * pf_trim_fastq[_pair] reports for the chunk.  stats: what pf_count_fastq / pf_maskcount_fastq report on the trimmed text (reads and
 * bases are of the reads handed on, of both files of a pair).  Timed as one launch of PF_K_TRIMCOUNT per call; unit: whole records
 * taken (of both files).  text: [host|dev] */
typedef struct pf_trim_plan {
    const pf_trim_step *steps;
    uint32_t n_steps;
    uint32_t phred;   /* 33 or 64 */
} pf_trim_plan;
/* the table by itself: read_off / read_len ([host|dev], room for one entry per whole record of the chunk -- at most n_bytes / 4)
 * receive *n_reads entries; *n_records = whole records taken.  A pair has one table per file, both of *n_reads entries: entry i of
 * both are the two records of one pair. */
int pf_trim_table_fastq(pf_ctx *, const char *text, uint64_t n_bytes, int final, const pf_trim_plan *plan, uint64_t *read_off, uint32_t *read_len,
                        uint64_t *n_reads, uint64_t *bytes_used, uint64_t *n_records, pf_trim_stats *stats, uint64_t *bad_record);
int pf_trim_table_fastq_pair(pf_ctx *, const char *text1, uint64_t n1, const char *text2, uint64_t n2, int final, const pf_trim_plan *plan,
                             uint64_t *read_off[2], uint32_t *read_len[2], uint64_t *n_reads, uint64_t bytes_used[2], uint64_t *n_records,
                             pf_trim_stats stats[2], uint64_t *bad_record);
int pf_count_fastq_trimmed(pf_ctx *, const char *text, uint64_t n_bytes, int final, const pf_trim_plan *plan, uint64_t *bytes_used,
                           pf_trim_stats *trim_stats, pf_count_stats *stats, uint64_t *bad_record);
int pf_count_fastq_pair_trimmed(pf_ctx *, const char *text1, uint64_t n1, const char *text2, uint64_t n2, int final, const pf_trim_plan *plan,
                                uint64_t bytes_used[2], pf_trim_stats trim_stats[2], pf_count_stats *stats, uint64_t *bad_record);
int pf_maskcount_fastq_trimmed(pf_ctx *, const char *text, uint64_t n_bytes, int final, const pf_trim_plan *plan, uint32_t low, uint32_t up,
                               uint64_t *bytes_used, pf_trim_stats *trim_stats, pf_maskcount_stats *stats, uint64_t *bad_record);
int pf_maskcount_fastq_pair_trimmed(pf_ctx *, const char *text1, uint64_t n1, const char *text2, uint64_t n2, int final, const pf_trim_plan *plan,
                                    uint32_t low, uint32_t up, uint64_t bytes_used[2], pf_trim_stats trim_stats[2], pf_maskcount_stats *stats,
                                    uint64_t *bad_record);
/* K-CLIP: adapter read-through clipped on the device in front of the steps of K-TRIM and K-TRIMCOUNT (csrc/pf_clip.hip; the rule:
 * csrc/pf_clip_rule.hpp).  A clip is state on the context, opened and closed like a count.  While one is open, pf_trim_fastq,
 * pf_trim_fastq_pair, pf_trim_table_fastq[_pair], pf_count_fastq[_pair]_trimmed and pf_maskcount_fastq[_pair]_trimmed clip first: the
 * interval of a read starts as [0, clip end) instead of [0, n), clip end 0 = dropped, and they accept n_steps == 0.  With none open
 * they are bit for bit what they were, the `no step is given` refusal included.  A single-ended call and file 1 of a pair use the
 * adapters of side 0 and 1, file 2 those of side 0 and 2.
 * The rule: a read of n bases with q[p] = (int)byte - phred, an adapter of m bases (16 .. 128 of ACGTacgt, at most 64 adapters).
 * Offset o aligns adapter position j with read position o + j, -(m - 16) <= o <= n - 16; the overlap [max(0, o), min(n, o + m)) holds
 * at least 16 positions.  Seed: the overlap holds 16 consecutive positions with at most `seed` (0 .. 8) mismatches, a read byte outside
 * ACGTacgt being one.  Score: per overlap position 0 for a read byte outside ACGTacgt, +60206 for equal bases (case folded), else
 * -10000 * max(q, 0); the best sum over contiguous sub-ranges, at least 0, must reach 100000 * score (1 .. 1000).  o* = the smallest
 * passing offset over the side's adapters: none -- untouched; o* <= 0 -- dropped; else clip end o*.  PARITY with Trimmomatic's
 * ILLUMINACLIP UNPINNED; knowingly different: the smallest offset over all adapters instead of the first found per adapter, no
 * overlaps below 16, N a full seed mismatch, no palindrome mode.
 * bases: the adapters one behind the other, adapter a = bases[adapter_off[a], adapter_off[a + 1]); adapter_off has n_adapters + 1
 * entries; side[a] = 0 (both files), 1 or 2.  All [host]; they are copied.  A second begin, an end or a stats_get without a begin, and
 * every value out of range: PF_ERR_ARG by name.  The statistics add up over all calls since the begin; a refused call adds nothing. */
typedef struct pf_clip_stats {   /* [0]: single-ended calls and file 1 of a pair; [1]: file 2 */
    uint64_t reads_clipped[2];      /* reads cut to o* > 0 bases */
    uint64_t reads_dropped[2];      /* reads with o* <= 0 */
    uint64_t bases_clipped[2];      /* n - clip end over both */
    uint64_t candidates_scored[2];  /* (adapter, offset) pairs whose seed held: the ones scored */
} pf_clip_stats;
int pf_clip_begin(pf_ctx *, const char *bases, const uint32_t *adapter_off, const uint8_t *side, uint32_t n_adapters, uint32_t seed, uint32_t score);
int pf_clip_stats_get(pf_ctx *, pf_clip_stats *stats);
/* the clip ends of the last pf_trim_fastq* / pf_trim_table_fastq* / pf_*_trimmed call, before another one is made: clip_end [host|dev]
 * receives n_records entries (at most the records that call took) of file 0 or 1 -- n untouched, 0 dropped.  A call that took no whole
 * record (or was refused) clipped none: n_records == 0 is PF_OK, more is refused by name.  What `trim --trimlog` counts its last column from. */
int pf_clip_last_ends(pf_ctx *, int file, uint32_t *clip_end, uint64_t n_records);
int pf_clip_end(pf_ctx *);
/* K-PALIN: palindrome mode beside simple mode (csrc/pf_clip.hip; the rule: csrc/pf_clip_rule.hpp, "PALINDROME MODE").  A clip opened
 * with pf_clip_begin_pairs holds prefix pairs as well: pair q is P1 = prefix_bases[prefix_off[2q], prefix_off[2q + 1]) and P2 =
 * [prefix_off[2q + 1], prefix_off[2q + 2]), both of one length 16 .. 128, 1 .. 8 pairs.  The simple adapters may be none
 * (n_adapters == 0).  seed serves both modes; score is simple mode's T, pair_score palindrome mode's Tp (1 .. 1000), pair_min the
 * fewest adapter bases A (1 .. 16); keep_both != 0 leaves file 2 of a clipped pair its first I* bases instead of dropping it.  While
 * such a clip is open the paired calls named above clip every pair by both modes: a read's clip end is the smaller of its simple clip
 * end and its pair end, pf_clip_last_ends hands out that final end, and reads_clipped / reads_dropped / bases_clipped of
 * pf_clip_stats describe it.  A pair with a read of more than 1024 bases is clipped by simple mode alone.  A single-ended call clips
 * with the simple adapters only (with none: nothing).  Refusals by name, as pf_clip_begin's.  pf_clip_pair_stats_get needs a clip
 * opened with pairs. */
typedef struct pf_clip_pair_stats {
    uint64_t pairs_clipped;      /* pairs with I* > 0 */
    uint64_t pairs_dropped;      /* pairs with I* == 0 */
    uint64_t pairs_too_long;     /* pairs with a read of more than 1024 bases: no candidate */
    uint64_t candidates_scored;  /* (prefix pair, I) examined whose seed held */
    uint64_t bases_clipped[2];   /* simple clip end - final clip end, per file: what this mode took beyond simple mode */
} pf_clip_pair_stats;
int pf_clip_begin_pairs(pf_ctx *, const char *bases, const uint32_t *adapter_off, const uint8_t *side, uint32_t n_adapters /* may be 0 */,
                        const char *prefix_bases, const uint32_t *prefix_off /* 2 * n_pairs + 1 */, uint32_t n_pairs,
                        uint32_t seed, uint32_t score, uint32_t pair_score, uint32_t pair_min, int keep_both);
int pf_clip_pair_stats_get(pf_ctx *, pf_clip_pair_stats *stats);
/* K-QC: a read quality report accumulated on the device (csrc/pf_qc.hip; the rule, the words of a table and the text of the report:
 * csrc/pf_qc_rule.hpp).  A report is state on the context, opened and closed as a clip is.  While one is open, pf_trim_fastq[_pair],
 * pf_trim_table_fastq[_pair], pf_count_fastq[_pair]_trimmed and pf_maskcount_fastq[_pair]_trimmed add every whole record they take to
 * the table (side, PF_QC_RAW) with the interval [0, n) and every record K-TRIM keeps to (side, PF_QC_KEPT) with its final interval,
 * the clip included; with a clip open as well, every record with clip end < n adds one to clip[min(clip end, 1024)] of its side.
 * Side 0: single-ended calls and file 1 of a pair; side 1: file 2.  Their outputs are what they are with no report open, and with
 * none open they launch and allocate nothing new.  phred (33 or 64) is the offset the tables are taken with, whatever a call's own.
 * pf_qc_fastq indexes one chunk by the chunk contract and the format clauses of pf_trim_fastq and adds its whole records to
 * (side, PF_QC_RAW) alone.  pf_qc_get: words [host] receives PF_QC_TABLE_WORDS uint64_t, pf_qc_clip_get PF_QC_CLIP_WORDS (all 0 when
 * no clip was open).  A table nothing was added to is all zero.  A second begin, and get / fastq / end without a begin: PF_ERR_ARG by name. */
#define PF_QC_TABLE_WORDS 9515u
#define PF_QC_CLIP_WORDS 1025u
enum { PF_QC_RAW = 0, PF_QC_KEPT = 1 };
int pf_qc_begin(pf_ctx *, uint32_t phred);
int pf_qc_get(pf_ctx *, int side, int stage, uint64_t *words);
int pf_qc_clip_get(pf_ctx *, int side, uint64_t *words);
int pf_qc_fastq(pf_ctx *, int side, const char *text, uint64_t n_bytes, int final, uint64_t *bytes_used, uint64_t *n_records, uint64_t *bad_record);
int pf_qc_end(pf_ctx *);
/* K-DEDUP: duplicate reads dropped on the device (csrc/pf_dedup.hip; the rule -- unit, key, decision, statistics: csrc/pf_dedup_rule.hpp).
 * A dedup is state on the context, opened and closed as a clip and a report are: a hash table in HBM that lives across the chunks of a
 * stream, and the number of units taken.  While one is open, pf_trim_fastq[_pair], pf_trim_table_fastq[_pair],
 * pf_count_fastq[_pair]_trimmed and pf_maskcount_fastq[_pair]_trimmed give every unit K-TRIM keeps (a record; for a pair record r of
 * both files, both kept) the 128-bit key of its raw sequence line(s) -- the first `bases` bases, 0 = the whole read -- and drop every
 * unit whose key an earlier unit of the stream had: its interval becomes empty in every file, as if MINLEN had dropped it, and
 * pf_trim_stats describes what is left.  They accept n_steps == 0 as with a clip open.  A refused call inserts nothing and does not
 * advance the unit counter.  With none open they launch and allocate nothing new.  initial_slots: 0 = default, rounded up to a power
 * of two, at least 64; the table grows by itself (2 * (entries + units of the call) <= slots before every call) and a table that
 * does not fit the free device memory is refused by name with the units reached (PF_ERR_OVERFLOW).
 * pf_dedup_stats_get: one pass over the table.  levels[c - 1] = keys with c copies, levels[9] = 10 or more.
 * pf_dedup_keys: the table by itself, for tests and tools -- n keys (two words each, a zero word counts as 1) as units
 * next_unit .. next_unit + n - 1 that all take part; keep[i] = 1 when key i had not been seen before (in the stream or in the call).
 * A second begin, and stats / keys / end without a begin: PF_ERR_ARG by name.  A probe that went round the table (impossible at half
 * load) is refused by name with PF_ERR_OVERFLOW by pf_dedup_stats_get and by pf_dedup_end, which frees the table all the same. */
typedef struct pf_dedup_stats { uint64_t units, unique, duplicates, max_copies, levels[10], slots, growths; } pf_dedup_stats;
int pf_dedup_begin(pf_ctx *, uint32_t bases /* 0 = whole read, else 16 .. 4096 */, uint64_t initial_slots /* 0 = default; rounded up to a power of two, at least 64 */);
int pf_dedup_stats_get(pf_ctx *, pf_dedup_stats *);
int pf_dedup_end(pf_ctx *);
int pf_dedup_keys(pf_ctx *, const uint64_t *keys /* [host|dev], 2n words */, uint64_t n, uint8_t *keep /* [host|dev], n */);
/* K-INFLATE: blocked gzip (BGZF: what bgzip, bcl2fastq2 and BCL Convert write) inflated on the device, where pf_*_fastq read their text.
 * The rule -- the member header, RFC 1951, the refusals by name -- is csrc/pf_inflate_rule.hpp; the decoder one lane runs is
 * csrc/pf_inflate_core.hpp, shared with the host.  One wavefront per member; the CRC-32 of every member's text is checked against
 * its trailer.  Timed as one launch of PF_K_INFLATE per call; unit: inflated bytes. */
typedef struct pf_inflate_stats {
    uint64_t members, bytes_in, bytes_out, blocks_stored, blocks_fixed, blocks_dynamic;
} pf_inflate_stats;
/* comp[0, n_bytes): whole BGZF members, member m = comp[member_off[m], member_off[m+1]); member_off has n_members + 1 entries.
 * out receives the members' texts one behind the other; *out_bytes = their sum.  out_cap too small: PF_ERR_OVERFLOW, *out_bytes = needed.
 * A refused member: PF_ERR_ARG, *bad_member = the smallest offender, pf_last_error names the clause ("pf_inflate_bgzf: member M of the
 * call: <clause>"); out is then unspecified.
 * comp, member_off, out: [host|dev] */
int pf_inflate_bgzf(pf_ctx *, const uint8_t *comp, uint64_t n_bytes, const uint64_t *member_off, uint64_t n_members,
                    char *out, uint64_t out_cap, uint64_t *out_bytes, pf_inflate_stats *stats, uint64_t *bad_member);

/* K-DEFLATE: text deflated to blocked gzip (BGZF) on the device.  The rule -- the parse, the coding, the block choice and the container,
 * each a function of the member's text alone -- is csrc/pf_deflate_core.hpp, shared with the host (csrc/pf_deflate_rule.hpp): a call
 * gives the bytes the host rule gives, member for member.  One block per member; the members go to slots, their sizes are scanned and
 * a second kernel packs them.  Timed as one launch of PF_K_DEFLATE per call; unit: bytes of text. */
typedef struct pf_deflate_stats { uint64_t members, bytes_in, bytes_out, blocks_stored, blocks_fixed, blocks_dynamic, literals, matches; } pf_deflate_stats;
/* text[0, n_bytes) cut into members of member_text bytes (1 .. 65280; the last may be shorter; n_bytes = 0: no member).  out receives
 * the members one behind the other, *out_bytes their sum; member_off (may be NULL) n_members + 1 offsets into out.
 * out_cap below n_bytes + 31 * members: PF_ERR_OVERFLOW by name with that bound.  text, out, member_off: [host|dev] */
int pf_deflate_bgzf(pf_ctx *, const char *text, uint64_t n_bytes, uint32_t member_text, uint8_t *out, uint64_t out_cap,
                    uint64_t *out_bytes, uint64_t *member_off, pf_deflate_stats *stats);

/* K-GUNZIP: a plain gzip member's deflate stream (what gzip and pigz write) inflated on the device.  One stream has no table of its
 * blocks, so it is cut into pieces at block starts that a search finds, every piece is decoded twice (count, then decode into 16-bit
 * symbols with markers for what lies in front of the piece) and the markers are resolved afterwards.  The rule -- the container, the
 * refusals by name, the same stages on the host -- is csrc/pf_gunzip_rule.hpp; what one lane runs is csrc/pf_gunzip_core.hpp.  Timed as
 * one launch of PF_K_GUNZIP per call; unit: inflated bytes. */
typedef struct pf_gunzip_result {
    uint64_t out_bytes;   /* bytes of text written (PF_ERR_OVERFLOW: needed) */
    uint64_t end_bit;     /* the last complete block boundary: where the next call starts */
    uint32_t final;       /* the call ended behind a final block: the trailer follows at the next byte boundary */
    uint32_t n_window;    /* bytes of the new window */
    uint32_t crc_raw;     /* the raw CRC-32 register (from zero, not inverted) of the call's text: the caller combines the calls' */
    uint32_t clause;      /* a refusal: the clause (pf_inflate::Clause, pf_gunzip::Clause) and the block boundary in front of it */
    uint64_t clause_bit;
} pf_gunzip_result;
typedef struct pf_gunzip_stats {
    uint64_t pieces_found, pieces_live, pieces_dead, markers, blocks_stored, blocks_fixed, blocks_dynamic, bytes_in, bytes_out;
    double stage_ms[5];   /* find, count, decode, window, resolve: filled when timing is on */
} pf_gunzip_stats;
/* comp[0, n_bytes) from start_bit on, a block start.  window[0, n_window): the last n_window <= 32768 bytes of the member's text so
 * far (0 at a member's start); new_window (32768 bytes, may be window) receives the last bytes of the text including this call's.
 * piece_bytes: the nominal piece stride in compressed bytes (0: 16384; at least 64).  The call stops at a final block or, when the
 * bytes end inside a block, at the last complete block boundary.  out_cap too small: PF_ERR_OVERFLOW, res->out_bytes = needed,
 * nothing written.  A refused stream: PF_ERR_ARG with res->clause and res->clause_bit, pf_last_error names the clause.
 * comp, window, out, new_window: [host|dev] */
int pf_inflate_gzip(pf_ctx *, const uint8_t *comp, uint64_t n_bytes, uint64_t start_bit, const uint8_t *window, uint32_t n_window,
                    uint32_t piece_bytes, char *out, uint64_t out_cap, uint8_t *new_window, pf_gunzip_result *res, pf_gunzip_stats *stats);

/* K-HETPAIR: the heterozygous k-mer pairs of a Smudgeplot-style check of the ploidy estimate, from the distinct canonical k-mers and
 * counters pf_count_finish / pf_kmc_decode leave on the device and the count table pf_upload_counts built from them (the rule is
 * csrc/pf_hetpair_rule.hpp; PARITY UNPINNED, Smudgeplot is not part of the build).  S = the keys with lo <= counter <= hi; a pair is
 * (x, y), x < y, both in S, one substitution apart as canonical k-mers, neither with another neighbour in S.  table: W * W uint64_t
 * cells, W = hi - lo + 1 <= 4096, table[(a - lo) * W + (b - lo)] = pairs with the counters a <= b; [host|dev], may be NULL.  The four
 * arrays (all given or all NULL) receive device arrays of *n_pairs entries in the order of x in `kmers`, released with pf_device_free
 * (NULL when there is no pair).  kmers, counts: [host|dev], distinct keys.  Needs a resident single-sample count table of the same k,
 * counted on both strands and uploaded from the same arrays (the caller's duty, as for K-MASK); each missing piece, lo < 1, lo > hi
 * and W > 4096 are PF_ERR_ARG by name.  n = 0: empty results. */
typedef struct pf_hetpair_stats {
    uint64_t kmers;          /* keys given */
    uint64_t in_range;       /* keys of S */
    uint64_t one_partner;    /* keys of S with exactly one distinct neighbour in S */
    uint64_t many_partners;  /* keys of S with two or more */
    uint64_t pairs;
} pf_hetpair_stats;
int pf_hetpairs(pf_ctx *, const uint64_t *kmers, const uint32_t *counts, uint64_t n, uint32_t k, uint32_t lo, uint32_t hi,
                uint64_t *table, uint64_t **pair_x_dev, uint64_t **pair_y_dev, uint32_t **cov_x_dev, uint32_t **cov_y_dev,
                uint64_t *n_pairs, pf_hetpair_stats *stats);
/* The table kernel of K-HETPAIR alone over compacted counters on the device (pairs with a counter outside [lo, hi] add nothing);
 * table: [host|dev].  Timed as a launch of PF_K_HETPAIR; unit: pairs. */
int pf_hetpair_table(pf_ctx *, const uint32_t *cov_x_dev, const uint32_t *cov_y_dev, uint64_t n_pairs, uint32_t lo, uint32_t hi, uint64_t *table);

int pf_copy_to_host(pf_ctx *, void *dst, const void *src_dev, size_t bytes);
/* Device memory of the caller's own (freed with pf_device_free), and a copy between any two places (host or device) on the launch
 * stream, waited for: what the host layer keeps the inflated text of `--gz` in between two calls. */
int pf_device_alloc(pf_ctx *, size_t bytes, void **out);
int pf_copy(pf_ctx *, void *dst, const void *src, size_t bytes);

/* K1/K2: builds the device hash table from the database records (exact k-mers as stored, any
 * order).  Records with count outside [min_count, max_count] are not retrievable, as in
 * CKMCFile::BinarySearch (kmc_file.cpp:1459).  both_strands mirrors GetBothStrands().
 * k = the database's k-mer length (CKMCFileInfo::kmer_length; it must equal the graph's, whichever of the two is uploaded
 * first): the table is addressed by the MINIMIZER of a key, not by a hash of the whole key, so that the k-mers of a unitig --
 * which CDBG::readCov asks for one after the other (src/CDBG.cpp:66-120) -- lie in the same few 128-B lines
 * (csrc/pf_device_common.hpp, "minimizer-local addressing").  [host|dev] */
int pf_upload_counts(pf_ctx *, const uint64_t *kmers, const uint32_t *counts, uint64_t n, uint32_t k, uint64_t min_count,
                     uint64_t max_count, int both_strands);
/* Gives the single-sample count table (and the coverage array joined from it) back: the context is as before the first
 * pf_upload_counts.  `ploidyfrost run-multi` calls it behind the last sample's second pass, before the coloured graph goes in. */
int pf_release_counts(pf_ctx *);
/* K-COV-JOIN again (it runs by itself when graph and table are both resident): every look-up CDBG::readCov(UnitigMap) makes in one
 * run of the reference -- one CheckKmer per graph k-mer (src/CDBG.cpp:66-120 inside :1187-1220) -- as one kernel launch.  For
 * callers that account for those look-ups per pass (bench.py's value_incl_join).  PF_ERR_ARG without a graph and a canonical table. */
int pf_join_counts(pf_ctx *);
/* The same in two halves: _begin launches the look-ups on a stream of their own (lowest priority) and returns; whatever the caller
 * runs next on the context that reads no coverage -- pf_bfs_candidates ... pf_replay_device: findSuperBubble -- shares the device
 * with them; _end waits.  Every reader of the joined array (pf_unitig_cov, pf_call_coverage) waits by itself, so _end may be left out. */
int pf_join_counts_begin(pf_ctx *);
int pf_join_counts_end(pf_ctx *);
/* K2+K3 composite of src/CDBG.cpp:38-56 for a batch of k-mers:
 * "if (!IsKmer(fwd)) reverse(); CheckKmer()".  found[i] = 0 when absent. [host|dev] */
int pf_lookup_kmers(pf_ctx *, const uint64_t *kmers, uint64_t n, uint32_t *counts, uint8_t *found);

/* ---- C1: CDBG::readCov(const UnitigMap&) (src/CDBG.cpp:66-120) for unitigs [u0, u1) ------ */
/* sum = sum of canonical counts over the unitig's k-mers, min = min(10000, counts),
 * miss = 1 if some k-mer is absent.  Arrays are indexed from u0.  The host does the one
 * division (mean = sum / len). Returns PF_ERR_MISSING_KMER after filling the arrays if
 * any miss flag is set. [host|dev] */
int pf_unitig_cov(pf_ctx *, uint32_t u0, uint32_t u1, uint64_t *sum, uint32_t *min, uint8_t *miss);
/* How pf_unitig_cov gets there: as soon as a graph and a canonical count table are both resident (whichever of
 * pf_upload_graph / pf_upload_counts comes second) the device joins them once -- every graph k-mer's count is written
 * to its position in graph order, a per-k-mer coverage SoA beside the sequence SoA (kernel PF_K_COV_JOIN; the
 * load-time counterpart of pf_build_adjacency).  pf_unitig_cov then streams that array: a segmented sum / min over
 * 4 contiguous bytes per k-mer instead of one random table access per k-mer.  pf_unitig_cov_probe is the same
 * function computed the other way -- every k-mer looked up in the hash table at call time -- kept for databases the
 * SoA cannot hold (max_count = 2^32 - 1) and as the independent check of the join (tests, measurements).
 * Identical results by construction. [host|dev] */
int pf_unitig_cov_probe(pf_ctx *, uint32_t u0, uint32_t u1, uint64_t *sum, uint32_t *min, uint8_t *miss);
/* The branch for a database built without canonical counting (GetBothStrands() == false, src/CDBG.cpp:94-117): every k-mer of
 * mappedSequenceToString() is looked up as it reads.  reverse = 0: the unitig as stored; 1: its reverse complement (the '-'
 * orientation).  pf_unitig_cov refuses such a table; pf_string_cov returns sum 0 / ok 1 for it without looking anything up, as
 * readCov(string) does (:34, :59). [host|dev] */
int pf_unitig_cov_exact(pf_ctx *, uint32_t u0, uint32_t u1, int reverse, uint64_t *sum, uint32_t *min, uint8_t *miss);

/* ---- S2: CDBG::extractSuperBubble_ptr (src/CDBG.cpp:253-415), pure part ------------------ */
typedef struct pf_bfs_record {
    uint32_t entrance;  /* oriented vertex s */
    uint32_t exit;      /* oriented vertex t, PF_NONE when outcome == PF_BFS_NONE */
    uint32_t n_seen;    /* |vec_km_seen| (full length, even when list not stored) */
    uint32_t n_list;    /* entries stored at list_off: seen[] for outcomes 1..3, the
                           cycle set for outcome 0 with flag_cycle */
    uint64_t list_off;  /* offset into the vertex pool */
    uint8_t outcome;    /* enum pf_bfs_outcome */
    uint8_t flag_cycle;
    uint8_t flag_tip;
    uint8_t strict;     /* accept only: the structural test of src/CDBG.cpp:765-782 passed */
    uint32_t pad_;
} pf_bfs_record;

enum pf_bfs_outcome {
    PF_BFS_NONE = 0,       /* stack ran empty: no exit (src/CDBG.cpp:373-414 applies) */
    PF_BFS_CYCLE_EXIT = 1, /* exit found, s is a successor of t  -> setNoBubble_ptr_cycle */
    PF_BFS_REJECT = 2,     /* exit found, cycle or tip inside     -> setNoBubble_ptr(seen, p) */
    PF_BFS_ACCEPT = 3      /* exit found, clean                   -> setNoBubble_ptr(p, seen) */
};

/* Candidates: every oriented vertex with out-degree > 1 (the order-dependent
 * `partner == NULL` gate of src/CDBG.cpp:206,211 is applied by the host during replay).
 * pf_count_candidates returns how many lie in unitigs [u0, u1); pf_bfs_candidates traverses
 * them, one wavefront each, and writes one record per candidate in ascending entrance
 * order plus the variable-length vertex lists into pool (pool_cap entries).
 * PF_ERR_OVERFLOW: *pool_used tells the size needed. [host|dev] */
int pf_count_candidates(pf_ctx *, uint32_t u0, uint32_t u1, uint64_t *n_candidates);
int pf_bfs_candidates(pf_ctx *, uint32_t u0, uint32_t u1, pf_bfs_record *records, uint64_t rec_cap,
                      uint32_t *pool, uint64_t pool_cap, uint64_t *n_records, uint64_t *pool_used);
/* The same with everything beyond the first (LDS, 128-entry) tier left to the caller: a long traversal is one chain of
 * dependent memory accesses (LIFO order fixes its result), which a host core walks two orders of magnitude faster than a lone
 * wavefront (~20 ns against ~2.4 us per vertex).  records / pool must be host memory; deferred[0 .. *n_deferred) = indices (into records) of those candidates,
 * whose records come back with only `entrance` set (exit = PF_NONE, outcome = PF_BFS_NONE, no list) for the caller to fill. */
int pf_bfs_candidates_split(pf_ctx *, uint32_t u0, uint32_t u1, pf_bfs_record *records, uint64_t rec_cap, uint32_t *pool,
                            uint64_t pool_cap, uint64_t *n_records, uint64_t *pool_used, uint32_t *deferred, uint64_t deferred_cap,
                            uint64_t *n_deferred);
/* pf_bfs_candidates_split in two steps, so that the copy of the records to the host (183 MB for the 5 M-unitig graph) runs
 * beside the caller's walk of the deferred traversals: _begin returns once the device tiers have run, with the deferred
 * candidates' indices and entrances (oriented vertices) and with records / pool on their way on a copy stream; _end waits for
 * them and marks the deferred records as pf_bfs_candidates_split does.  Between the two calls the caller must not touch
 * records / pool; it may call pf_side_components(records = NULL). */
int pf_bfs_candidates_begin(pf_ctx *, uint32_t u0, uint32_t u1, pf_bfs_record *records, uint64_t rec_cap, uint32_t *pool, uint64_t pool_cap,
                            uint64_t *n_records, uint64_t *pool_used, uint32_t *deferred, uint32_t *deferred_entrance, uint64_t deferred_cap,
                            uint64_t *n_deferred);
int pf_bfs_candidates_end(pf_ctx *);

/* ---- A1: SeqAlign::needlemanWunch + traceback (src/SeqAlign.cpp:480-549, 306-478) ------- */
/* One job = one pairwise alignment A x B.  Sequences are ASCII over {A,C,G,T,-}
 * ('-' only in A, when A is a row of an earlier alignment).  For every job the device
 * performs the full-matrix fill (scores in `int = long + double` arithmetic, +1 same-direction
 * bonus, look-ahead rule, all tying directions flagged) and the all-co-optimal traceback with
 * the shrinking 5-gap-open budgets, and returns the kept alignments in traceback order. */
typedef struct pf_align_job {
    uint64_t a_off, b_off; /* offsets into the text buffer */
    uint32_t a_len, b_len;
} pf_align_job;

typedef struct pf_align_hit {
    uint64_t text_off;   /* aligned rows: a at text_off, b at text_off + len (out_text) */
    uint64_t gap_off;    /* gap_pos entries at gap_off (out_gaps), traceback order */
    uint32_t len;        /* aligned length */
    uint32_t n_gaps;
    int64_t score;       /* variantAnalyze score (src/SeqAlign.cpp:255) */
    uint32_t n_pos;      /* variant positions */
    uint32_t n_indel;
} pf_align_hit;

/* hits of job j are hits[hit_first[j] .. hit_first[j] + hit_count[j]) (both arrays have n_jobs
 * entries; jobs are published in completion order, so the ranges are not sorted by j).
 * PF_ERR_OVERFLOW when a capacity is too small: the sizes needed are returned in used[3] =
 * {hits, text bytes, gap entries}. [text, jobs and all outputs: host|dev] */
int pf_align_batch(pf_ctx *, const char *text, uint64_t text_len, const pf_align_job *jobs, uint32_t n_jobs,
                   double match, double mismatch, double gap, uint64_t *hit_first, uint32_t *hit_count,
                   pf_align_hit *hits, uint64_t hit_cap, char *out_text, uint64_t text_cap, uint32_t *out_gaps,
                   uint64_t gap_cap, uint64_t used[3]);

/* ---- A1 complete: SeqAlign::SequenceAlignment (src/SeqAlign.cpp:550-640) -------------------- */
/* One task = one bubble: its N >= 2 path strings in the order the host sorted them.  The device
 * runs the whole multiple alignment for it on one wavefront: needlemanWunch + traceback of rows 0
 * and 1, then rows 2..N-1 progressively against row 0 of every kept alignment (re-opening the new
 * gaps in the older rows, re-scoring them as variantAnalyze does, keeping the best-ranked
 * candidates), and finally the selection ladder of compareStrPair (src/SeqAlign.cpp:8-236).
 * A path is either a slice of `text` (ASCII ACGT) or, with ov != PF_NONE, the whole oriented
 * unitig ov decoded from the packed graph (mappedSequenceToString). */
typedef struct pf_bubble_path {
    uint64_t text_off;
    uint32_t len;
    uint32_t ov;
} pf_bubble_path;

typedef struct pf_bubble_task {
    uint64_t path_first; /* index into paths */
    uint32_t n_paths;
    uint32_t pad_;
} pf_bubble_task;

typedef struct pf_bubble_site { /* one column with partition[col].back() > 0 */
    uint32_t col;
    uint8_t is_indel; /* col is in indel_pos (opens an indel) */
    uint8_t maxnum;   /* number of allele groups */
    uint16_t pad_;
} pf_bubble_site;

typedef struct pf_bubble_result {
    uint64_t rows_off;  /* n_rows * n_cols chars, row-major, in out_text */
    uint64_t site_off;  /* n_sites records in out_sites */
    uint64_t group_off; /* n_sites * n_rows bytes in out_groups: 1-based allele group of every row */
    uint64_t ilen_off;  /* n_indel_len u32 in out_ilen (indel_len_vec) */
    uint32_t n_rows;    /* 0: no alignment survived (the reference skips the bubble, src/CDBG.cpp:1254) */
    uint32_t n_cols;
    uint32_t n_sites;
    uint32_t n_indel_len;
} pf_bubble_result;

/* PF_ERR_OVERFLOW when a pool is too small: used[4] = {text bytes, sites, group bytes, ilen entries}
 * tells the sizes needed.  [all pointers host|dev] */
int pf_align_bubbles(pf_ctx *, const char *text, uint64_t text_len, const pf_bubble_path *paths, uint64_t n_paths,
                     const pf_bubble_task *tasks, uint32_t n_tasks, double match, double mismatch, double gap,
                     pf_bubble_result *results, char *out_text, uint64_t text_cap, pf_bubble_site *out_sites,
                     uint64_t site_cap, uint8_t *out_groups, uint64_t group_cap, uint32_t *out_ilen, uint64_t ilen_cap,
                     uint64_t used[4]);

/* ---- C2: CDBG::readCov(const string&, low, up) (src/CDBG.cpp:29-60) ---------------------- */
/* strings are ASCII ACGT, string i = text[str_off[i] .. str_off[i+1]).  sum[i] = sum of
 * canonical counts, ok[i] = 0 if any count is outside (low, up) (sum forced to 0), miss[i] = 1 if
 * a k-mer is absent. [host|dev] */
int pf_string_cov(pf_ctx *, const char *text, const uint64_t *str_off, uint32_t n_str, uint32_t low, uint32_t up,
                  uint64_t *sum, uint8_t *ok, uint8_t *miss);

/* ---- P1-P4 + O1 resident: CDBG::ploidyEstimation_ptr (src/CDBG.cpp:1101-1705) between the commit replay and the files -------
 * The caller keeps what is sequential by construction -- the commit replay of findSuperBubble and the light pass of the driver
 * loop that decides which endpoint sides are still open when reached (:1146-1186, 1656-1679) -- and the file system.  Everything
 * else runs on the device and comes back as text: owner / coverage-gate scan, path enumeration and sorting (strict: sortSeq_simple
 * :482-551; branching: two-stack walk :1364-1412 + sortSeq_branching :417-480), SequenceAlignment, per-site strings and their
 * readCov (:1448-1600, 29-60), and the rows of the ten result files with `ostream << double` formatting (:1259, 1303-1340,
 * 1552-1652).  Call order: pf_call_set_state, pf_call_coverage, pf_call_scan, pf_call_resolve (or pf_call_sides + pf_call_select), then pf_call_run /
 * pf_call_fetch per batch.  Single-sample path (CDBG); the colored twin keeps pf_align_bubbles + pf_string_cov_colored. */

/* The colored twin, CCDBG::ploidyEstimation_ptr (src/CCDBG.cpp:2759-3531), on the same pipeline.  pf_call_set_colours (once per
 * graph, after pf_upload_counts_colored) hands over what the calling phase asks of the colour sets: full_mask = the colours on every
 * k-mer of unitig u as (n_colors + 63) / 64 64-bit words per unitig (colour c = bit c % 64 of word u * words + c / 64); size_total[u] = UnitigColors::size() with the unitig's own mapping; and for a colour on part of a unitig one
 * bit per k-mer, reference orientation: entries part_first[u] .. part_first[u + 1] (N + 1 prefix) = {part_colour[e], first word
 * part_word[e] in part_bits}.  [host|dev]  With colours set, pf_call_coverage leaves readCovUni (src/CCDBG.cpp:123-156) of every
 * (colour, unitig) resident; pf_call_scan applies the per-colour gates of :2838-2931 (its lower / upper arguments are ignored:
 * pf_call_set_cutoffs gives one pair per colour, before every pf_call_scan) and the colored sortSeq_simple (:368-480); K-PATHS
 * records the unitigs each bubble's walks visit, K-SITES maps every site string to its unitig (findUnitig, :3251, 3390), asks the
 * colour sets which colours cover it (UnitigColors::contains) and reads every colour's count of its k-mers from the joined table
 * (readCov(string, low, up, colour), :89-122); K-TEXT writes one row per colour that sees two allele groups or more, with the
 * colour id and the largest Cramer's V over the colour pairs (:330-366, 2964-3059, 3285-3339).  n_colors = 0: back to the
 * single-sample path.  The -t > 1 format (pf_call_set_format) and pf_call_peek are the single-sample path's. */
int pf_call_set_colours(pf_ctx *, uint32_t n_colors, const uint64_t *full_mask, const uint64_t *size_total, const uint32_t *part_first,
                        const uint32_t *part_colour, const uint64_t *part_word, const uint64_t *part_bits, uint64_t n_part, uint64_t n_words);
int pf_call_set_cutoffs(pf_ctx *, uint32_t n_colors, const uint32_t *lower, const uint32_t *upper);

/* T1: the MyUnitig state after findSuperBubble (src/MyUnitig.hpp:37-130): b bits; plus / minus partners (0 = NULL, id = u + 1).
 * n_unitigs entries each. [host|dev] */
int pf_call_set_state(pf_ctx *, const uint8_t *flags, const uint32_t *plus, const uint32_t *minus);
/* Which of the reference's two text formats the rows follow: 0 (default) = its `-t 1` functions (ids and var_count from 1,
 * allele_frequency.txt in site order: src/CDBG.cpp:222-252, 1259-1340, 1552-1652); 1 = its `-t > 1` functions (BubbleId and
 * var_count from 0 -- fetch_add returns the old value, :1829, 2056 --, the allele_frequency rows of a bubble grouped by arity,
 * bi then tri then tetra then, in the strict branch only, penta, rows of other arities absent: :2158-2162, 2550).  Row ORDER
 * across bubbles is the deterministic `-t 1` order in both (the reference's own order with threads depends on timing). */
int pf_call_set_format(pf_ctx *, int reference_mt);
/* S1, second half: the rows of <outpre>_super_bubble.txt (src/CDBG.cpp:222-252) from that state, formatted on the device: one row
 * `BubbleId<TAB>Entrance<TAB>Strand<TAB>Exit<TAB>isSimple<TAB>isComplex` per open endpoint side in unitig order, ids from 1 (the
 * header line is the caller's).  colored_rule = 1: CCDBG's rule -- an open unitig lists every side whose partner is set, self
 * included (src/CCDBG.cpp:2106-2132).  pf_superbubble_fetch copies the text out on a stream of its own (any thread). */
int pf_superbubble_rows(pf_ctx *, int colored_rule, uint64_t *n_rows, uint64_t *text_len);
int pf_superbubble_fetch(pf_ctx *, char *dst, uint64_t len);
/* C1 for every unitig into device-resident arrays the scan reads (pf_unitig_cov / pf_unitig_cov_exact without the copy back; a
 * missing k-mer is reported by the scan only where the driver loop reads that unitig's coverage). */
int pf_call_coverage(pf_ctx *);

typedef struct pf_call_side { /* one open endpoint side, in the driver loop's order: unitig ascending, '+' side first */
    uint32_t u;          /* unitig index */
    uint32_t exit_ov;    /* the bubble's other endpoint as an oriented vertex; PF_NONE: not found (err = 2) */
    uint32_t err_unitig; /* err = 1: the unitig with a k-mer missing from the count table */
    uint8_t plus_side;
    uint8_t kind;        /* 1 complex (skipped, :1163), 2 the other endpoint owns the bubble (:1190, 1352), 3 owner: called here */
    uint8_t aligned;     /* kind 3: passes the coverage gate of the strict branch (:1210-1220); branching bubbles always do */
    uint8_t err;         /* 0, 1 missing k-mer, 2 exit unreachable -- raised by the caller only if the side is still open */
} pf_call_side;
/* part A of the driver loop for every open side, from static state only; *n_sides = number of records */
int pf_call_scan(pf_ctx *, uint32_t lower, uint32_t upper, uint64_t *n_sides);
int pf_call_sides(pf_ctx *, pf_call_side *out, uint64_t cap); /* [host|dev] */
/* part B of the driver loop on the device, exactly: which sides are still open when their unitig comes up (a handled owner closes
 * the side its exit faces, :1656-1679) is a recursion over smaller indices, settled by rounds of a monotone propagation instead of
 * a walk over the sides.  Leaves the selection (the called bubbles, in output order) in the context.  *err = 1 / 2 with *err_unitig
 * when the first open side in order carries a missing k-mer / an unreachable exit: the reference exits there. */
int pf_call_resolve(pf_ctx *, uint64_t *n_bubbles, uint32_t *err, uint32_t *err_unitig);
/* the same verdict from the caller (it walked pf_call_sides' records itself): the records, ascending, whose bubble is called [host|dev] */
int pf_call_select(pf_ctx *, const uint32_t *side_index, uint64_t n_bubbles);

#define PF_CALL_STREAMS 10
enum pf_call_stream { /* <outpre>_<name>.txt */
    PF_OUT_ALLELE_FREQUENCY = 0, PF_OUT_ALIGNSEQ = 1, PF_OUT_BIFRE = 2, PF_OUT_TRIFRE = 3, PF_OUT_TETRAFRE = 4, PF_OUT_PENTAFRE = 5,
    PF_OUT_BICOV = 6, PF_OUT_TRICOV = 7, PF_OUT_TETRACOV = 8, PF_OUT_PENTACOV = 9
};
typedef struct pf_call_result {
    uint64_t text_len[PF_CALL_STREAMS]; /* bytes of each stream this batch produced */
    uint64_t allele[4];                 /* sites with 2, 3, 4, 5 alleles */
    uint64_t core_cov, core_num;        /* coreCov / coreNum (:1261-1262) */
    uint64_t n_called;                  /* bubbles whose alignment left rows: var_count advances by this */
    uint64_t align_jobs, site_strings, n_branching;
    uint64_t snp_jobs, pair_jobs, wave_jobs; /* of align_jobs: finished by K-SNP, by K-PAIR, sent to K-BUBBLE */
    uint64_t stack_jobs;                     /* ... finished by K-STACK (paths of one length, alignment = the paths stacked) */
    uint64_t alignseq_packed_len;            /* pf_call_set_alignseq_packed: bytes stream PF_OUT_ALIGNSEQ takes in the slab (text_len keeps the text's) */
    uint64_t numeric_packed;                 /* pf_call_set_numeric_packed: 1 when the slab's fetches deliver the numeric streams at four bits a character */
} pf_call_result;
#define PF_CALL_SLABS 4 /* text slabs of a context: a slab is free again once pf_call_fetch has copied it */
#define PF_CALL_LANES 4 /* aligned ranges a context keeps resident side by side (pf_call_align_lane) */
/* Bubbles [t0, t1) of the selection (at most 2^24): everything up to the text of the ten streams, left in slab 0 .. 3 of the
 * context; var_count_base = bubbles called by earlier batches.  complex_size = -z (bounds the walk stacks). */
int pf_call_run(pf_ctx *, int slab, uint64_t t0, uint64_t t1, uint64_t var_count_base, uint32_t complex_size, double match,
                double mismatch, double gap, pf_call_result *out);
/* The same in two steps, for a bubble list cut over several GPUs: a rank learns how many of its bubbles are
 * called (pf_call_align: paths, alignment, site coverages; fills n_called, align_jobs, site_strings, n_branching), the ranks
 * exchange those counts, and only then is the text written with the rank's var_count_base (pf_call_text: text_len, allele, core_*). */
int pf_call_align(pf_ctx *, uint64_t t0, uint64_t t1, uint32_t complex_size, double match, double mismatch, double gap,
                  pf_call_result *out);
int pf_call_text(pf_ctx *, int slab, uint64_t var_count_base, pf_call_result *out);
/* alignseq.txt is more than half of the text of a pass and every row of a bubble repeats the bubble's four numbers in front of a row
 * over five letters.  on != 0: the pf_call_text* calls that follow leave stream PF_OUT_ALIGNSEQ of a slab PACKED -- an index, then per
 * bubble one header and its rows at 3 bits per character (csrc/pf_alnpack.hpp: layout, and the host routine that writes the text out
 * of it, pf::alnpack_expand) -- 2.5 x fewer bytes over PCIe.  pf_call_result.text_len[PF_OUT_ALIGNSEQ] stays the length of the TEXT
 * (file offsets); .alignseq_packed_len is what the stream takes in the slab, i.e. the length to pass to pf_call_fetch /
 * pf_call_fetch_slab for it.  Default off. */
int pf_call_set_alignseq_packed(pf_ctx *, int on);
/* The other nine streams are numbers: text over sixteen characters -- the digits, '.', tab, newline, '-', 'e', '+' -- and, with
 * alignseq packed, half of what a pass sends over PCIe.  on != 0: the pf_call_text* calls that follow leave a second form of the slab
 * for the fetches (K-NIB): every numeric stream at FOUR BITS a character (first character in the low nibble of a byte; code c of
 * "0123456789.\t\n-e+"), PF_NUMERIC_PACKED_LEN(text_len) bytes; alignseq as before, its length rounded up to 16; and, behind the ten
 * streams, 16 bytes whose first word has bit s set when stream s holds a character outside the sixteen ("nan", "inf": a frequency
 * of 0 / 0) -- that stream's nibbles are then not its text, and pf_call_fetch_text hands its text over as K-TEXT wrote it.
 * pf_call_fetch / pf_call_fetch_slab / pf_call_fetch_range speak of this form (lengths as above; pf_call_fetch_slab with every
 * stream at its full length delivers the 16 bytes of the tail as well); pf_call_result.text_len stays the text's, .numeric_packed
 * says the form is there.  Default off. */
#define PF_NUMERIC_PACKED_LEN(text_len) (((((uint64_t)(text_len)) + 1) / 2 + 15) & ~15ull)
int pf_call_set_numeric_packed(pf_ctx *, int on);
int pf_call_fetch_text(pf_ctx *, int slab, int stream, char *dst, uint64_t len);
/* Takes the device buffers pf_call_align(_lane) would take on its first call for ranges of up to n_bubbles bubbles -- to be called
 * beside the load, so that a one-shot run does not pay its first alignment launch with two dozen allocations.  A hint: sizes that
 * turn out too small grow in pf_call_align as before.  Needs nothing but the context: it may run on a helper thread while another
 * thread loads graph and count table into the same context (pf_gfa_parse, pf_upload_graph, pf_kmc_decode, pf_upload_counts) -- it
 * touches none of what those calls read or write; the first pf_call_* call of the run must come after it has returned. */
int pf_call_reserve(pf_ctx *, uint64_t n_bubbles, uint32_t complex_size);
/* The same for the first n_lanes lanes (1 .. PF_CALL_LANES; pf_call_reserve takes two): a caller that aligns several ranges side by
 * side (pf_call_align_lane below) takes every lane's working set beside the load. */
int pf_call_reserve_lanes(pf_ctx *, uint64_t n_bubbles, uint32_t complex_size, int n_lanes);
/* The same for the text stage: what the first pf_call_text_range(_lane) of a run would take for pieces of up to piece_bubbles
 * bubbles (its two streams, the size tables, the text slabs by an estimate for k = 31), and K-TEXT's two passes once over no bubbles on
 * each stream: the first launch of a kernel that spills pays for the queue's scratch (2 ms inside a first piece otherwise).
 * pf_call_reserve does the same for K-BUBBLE's class streams (13 ms of a first PloidyEstimation at 5 M unitigs).  Beside the load
 * like pf_call_reserve (single-sample path; with colours, after pf_call_set_colours). */
int pf_call_reserve_text(pf_ctx *, uint64_t piece_bubbles);
/* What pf_call_align(_lane) left resident for the bubbles of its range, before any text is made of it -- the kernel-level view the
 * parity tests hold against SeqAlign::SequenceAlignment (src/SeqAlign.cpp:550-640) bubble by bubble: per bubble its endpoints and,
 * for a strict one, its sorted inner unitigs with their mean coverages (sortSeq_simple, src/CDBG.cpp:482-551); its pf_bubble_result
 * (aligned rows, variant columns, allele groups, indel lengths: offsets into the pools below, as pf_align_bubbles returns them;
 * pf_bubble_site.pad_ of a branching bubble's site = 1 when every site string passed readCov's range test, src/CDBG.cpp:1548-1551);
 * and for a branching bubble, from sv[sv_off[bubble]], per site maxnum group coverages and their sum (src/CDBG.cpp:1527-1551).
 * cap[5] / used[1..5]: row text bytes, sites, group bytes, indel lengths, site values; used[0] = bubbles.  All pointers NULL:
 * sizes only.  [host] */
typedef struct pf_call_bubble {
    uint32_t entrance_ov, exit_ov;
    uint32_t strict, n_inner;
    uint32_t inner[4];
    double cov[4], core_mean, cov_sum;
} pf_call_bubble;
int pf_call_peek(pf_ctx *, int lane, pf_call_bubble *bubbles, pf_bubble_result *results, uint64_t *sv_off, uint64_t bubble_cap, char *text,
                 pf_bubble_site *sites, uint8_t *groups, uint32_t *ilen, double *sv, const uint64_t cap[5], uint64_t used[6]);
/* K-TEXT for bubbles [first, first + count) of the batch pf_call_align left resident: one large alignment launch (its kernels'
 * tails are paid once) can be formatted, fetched and written in pieces.  var_count_base is the same for every piece: the bubbles
 * called before the aligned batch; out->n_called = those called inside the piece. */
int pf_call_text_range(pf_ctx *, int slab, uint64_t first, uint64_t count, uint64_t var_count_base, pf_call_result *out);
/* The two with a choice of where the aligned batch lies ("lane" 0 .. PF_CALL_LANES - 1; the calls above use lane 0): the rows of
 * one range of bubbles are formatted from one host thread (pf_call_text_range_lane: a stream, scratch and counters of its own)
 * while others align the next ranges into other lanes -- the copy of the text to the host, the slowest stage of a large pass,
 * then runs beside the alignment kernels instead of after them.  A lane owns its results AND the working set of its alignment
 * (lists, pools, per-wavefront scratch, counters, streams), so pf_call_align_lane calls on DIFFERENT lanes may run at the same time
 * from different host threads: every kernel of a range ends in a tail of a few slow bubbles, which the kernels of the next range
 * fill.  One pf_call_text_range_lane at a time; never two calls on the same lane.  Their error messages are set under a lock, and
 * pf_last_error hands every calling thread a copy of its own. */
int pf_call_align_lane(pf_ctx *, int lane, uint64_t t0, uint64_t t1, uint32_t complex_size, double match, double mismatch,
                       double gap, pf_call_result *out);
int pf_call_text_range_lane(pf_ctx *, int lane, int slab, uint64_t first, uint64_t count, uint64_t var_count_base,
                            pf_call_result *out);
/* The count pass of pf_call_text_range_lane alone: text_len, allele, core_* and n_called of the range, nothing written.  A rank of a
 * sharded run learns the sizes of its whole slice with it, the ranks exchange them, and the slice is then written piece by piece
 * (pf_call_text_range_lane) at offsets that are known -- format, fetch and file copy of consecutive pieces side by side. */
int pf_call_text_sizes(pf_ctx *, int lane, uint64_t first, uint64_t count, uint64_t var_count_base, pf_call_result *out);
/* Copies the first len bytes of one stream of a slab to dst (host memory, pinned for speed) on a stream of its own: may be
 * called from another thread while pf_call_run fills the other slab. */
int pf_call_fetch(pf_ctx *, int slab, int stream, char *dst, uint64_t len);
/* All PF_CALL_STREAMS streams of a slab, packed one after the other into dst (len[s] bytes of stream s): the copies are issued
 * together and waited for once. */
int pf_call_fetch_slab(pf_ctx *, int slab, char *dst, const uint64_t *len);
/* The same packed slab in byte ranges, without waiting: range `slot` (0 / 1, alternating) is complete when pf_call_fetch_wait(slot)
 * returns, so that the caller copies one range into its files while the next crosses PCIe (a rank's one large slab of a sliced run). */
int pf_call_fetch_range(pf_ctx *, int slab, uint64_t first_byte, char *dst, uint64_t len, int slot);
int pf_call_fetch_wait(pf_ctx *, int slot);
/* O1's number formatting alone (test hook): text + 32 * i receives printf("%g", values[i]) without terminator, len[i] its length
 * [host|dev] */
int pf_format_doubles(pf_ctx *, const double *values, uint64_t n, char *text, uint8_t *len);

/* ---- K-CC: which traversal records may be committed side by side (pf_cc.hip) ------------------------------------------
 * The commits of findSuperBubble are order-dependent (src/CDBG.cpp:206-214: candidate entrances in unitig order behind the
 * `partner == NULL` gate), but two records whose footprints -- the unitig sides they can touch -- are disjoint commute.
 * pf_side_components adds the records of one slice of a pass to a union-find over the 2N sides (reset != 0 starts a pass):
 *   records == NULL: the n_records records and the vertex pool the last pf_bfs_candidates* call left on the device;
 *   otherwise records / pool [host|dev] as pf_bfs_candidates returns them (list_off into pool).
 *   extra: n_extra records [host|dev] with lists in extra_pool -- the traversals a caller of pf_bfs_candidates_split walked
 *   itself; they add their footprints only (their labels come from their entrances like everyone's).  A second call with
 *   records == NULL for the same K-BFS call adds only its `extra` (the device-resident records went in with the first).
 * pf_replay_order then labels every record of that slice with its component and deals the components into n_classes (<= 1024)
 * work units: order[n_records] = record indices grouped by class, ascending inside a class; class_off[n_classes + 1] (host);
 * labels (optional, [host|dev]) = the component label of each record's entrance side.  A record naming a vertex outside the
 * graph or a list outside its pool is refused (PF_ERR_ARG). */
int pf_side_components(pf_ctx *, int reset, const pf_bfs_record *records, uint64_t n_records, const uint32_t *pool, uint64_t pool_len,
                       const pf_bfs_record *extra, uint64_t n_extra, const uint32_t *extra_pool, uint64_t extra_pool_len);
int pf_replay_order(pf_ctx *, uint32_t n_classes, uint32_t *order, uint32_t *class_off, uint32_t *labels);

/* The commits on the device.  After pf_side_components over ALL records of a pass (one call with reset != 0, records == NULL:
 * the records pf_bfs_candidates_resident left on the device; `extra` = the traversals the caller walked itself), every component
 * of at most small_limit list entries is committed by one device thread, in record order, into the context's T1 state
 * (MyUnitig bits and partner slots: what pf_call_set_state uploads).  Components above the limit and components holding an
 * `extra` record are left to the caller: pf_replay_device returns how many device-resident records they have (and their list
 * entries), pf_replay_big_fetch hands them over (index[] = their positions among the records, ascending; records with list_off
 * into pool), the caller commits them together with its own records on a zeroed state of its own and passes what it changed to
 * pf_replay_finish: sides[] (2u = plus side of unitig u, 2u + 1 = minus side), the partner slot of each and its per-side flag
 * byte (csrc/host/pf_state_ops.hpp: S_LINK, S_STRICT, S_COMPLEX, S_NON_SUPER).  pf_replay_finish merges the per-side bytes into
 * MyUnitig's and leaves the state resident for pf_superbubble_rows / pf_call_scan; pf_call_get_state copies it to the host. */
/* The candidates the device tiers give up on (traversals of more than 128 vertices: the caller walks them on host cores) are also
 * reported AHEAD of the call's return: *list = cap entries of pinned host memory, zeroed by THIS call (call it once per pass,
 * before the threads that poll the list are started), that the next pf_bfs_candidates* call of this context with a `deferred` array
 * fills while its kernels run -- entry = entrance (oriented vertex) << 32 | (candidate index + 1), in no particular order -- so that
 * the caller's walkers start on the first long traversal while the device is still busy instead of after the call has returned.  A
 * pf_bfs_candidates_resident that repeats itself after a pool overflow writes the list again from its first slot.  An entry is a NOTICE, written when a traversal reaches 48 vertices: the
 * traversal goes on on the device and may yet end there (it is then absent from `deferred`, and the caller drops its walk); every
 * candidate of `deferred` has an entry unless the list ran out of room.  pf_bfs_live_count: the entries the last call wrote (may
 * exceed cap: the surplus was dropped).  cap = 0 switches the list off. */
int pf_bfs_live_deferred(pf_ctx *, uint64_t cap, volatile uint64_t **list);
int pf_bfs_live_count(pf_ctx *, uint64_t *n);
int pf_bfs_candidates_resident(pf_ctx *, uint32_t u0, uint32_t u1, uint64_t *n_records, uint64_t *pool_used, uint32_t *deferred,
                               uint32_t *deferred_entrance, uint64_t deferred_cap, uint64_t *n_deferred);
/* Takes the device buffers the first pf_side_components / pf_replay_device pass over n_records records would take (a hint, to be
 * called beside the load like pf_call_reserve; the adjacency must be resident). */
int pf_find_reserve(pf_ctx *, uint64_t n_records);
int pf_replay_device(pf_ctx *, uint32_t complex_size, uint32_t small_limit, uint64_t *n_big, uint64_t *big_entries);
/* Colored path (CCDBG): the colour gate of the accept commit (src/CCDBG.cpp:2530-2621) reads, per unitig, the set of colours
 * present on every k-mer (full_mask: (n_colors + 63) / 64 words per unitig, as for pf_call_set_colours), UnitigColors::size() with the unitig's own mapping, and how many colours the pair encoding stores as
 * "full" [host|dev].  Set once per graph; pf_side_components and pf_replay_device then apply the colored commits
 * (n_colors == 0: back to the single-sample ones). */
int pf_replay_set_colours(pf_ctx *, uint32_t n_colors, const uint64_t *full_mask, const uint64_t *size_total, const uint32_t *n_full_enc);
int pf_replay_big_fetch(pf_ctx *, uint32_t *index, pf_bfs_record *records, uint32_t *pool);
int pf_replay_finish(pf_ctx *, const uint32_t *sides, const uint32_t *links, const uint8_t *side_flags, uint64_t n_patch);
int pf_call_get_state(pf_ctx *, uint8_t *flags, uint32_t *plus, uint32_t *minus);

/* ---- colored (multi-sample) coverage: reference src/CCDBG.cpp ------------------------------------- */
/* CCDBG::CCDBG (src/CCDBG.cpp:13-43) opens one KMC database per colour.  Here the records of all colours
 * are joined into one HBM table keyed by the stored k-mer with one count per colour, so a k-mer costs one
 * random access whatever the number of colours.  kmers[c] / counts[c]: n[c] records of colour c (exact
 * k-mers as stored, any order); min_count / max_count / both_strands per colour as in pf_upload_counts.
 * Requires pf_upload_graph first (k).  [host|dev per array] */
#define PF_MAX_COLORS_TABLE 1024  /* colours of the joined table, K-COV-C and K-STRCOV-C */
#define PF_MAX_COLORS PF_MAX_COLORS_TABLE /* colours of the resident calling pipeline (pf_call_set_colours) and of the commits on the device
                                     (pf_replay_set_colours): colour sets of (n_colors + 63) / 64 words, a lane per colour of a word in K-SITES */
int pf_upload_counts_colored(pf_ctx *, uint32_t n_colors, const uint64_t *const *kmers, const uint32_t *const *counts,
                             const uint64_t *n, const uint64_t *min_count, const uint64_t *max_count, const int *both_strands);
uint32_t pf_num_colors(const pf_ctx *);
/* CCDBG::readCovUni (src/CCDBG.cpp:123-156) for unitigs [u0, u1) and every colour at once; arrays are
 * colour-major: x[c * (u1 - u0) + (u - u0)].  sum / min / max over the k-mers colour c's database holds,
 * miss = 1 when it lacks one.  readCovUni(u, low, up, c) == (sum / len, true) iff !miss && min > low &&
 * max < up, else (0, false) -- the caller applies its cutoffs.  [host|dev] */
int pf_unitig_cov_colored(pf_ctx *, uint32_t u0, uint32_t u1, uint64_t *sum, uint32_t *min_count, uint32_t *max_count,
                          uint8_t *miss);
/* pf_unitig_cov_colored streams a colour-major per-k-mer coverage SoA that the device joins once when graph and databases are
 * both resident (as pf_unitig_cov does, see there); this is the same function with every k-mer looked up at call time -- the
 * independent check, and the route for a max_count of 2^32 - 1.  [host|dev] */
int pf_unitig_cov_colored_probe(pf_ctx *, uint32_t u0, uint32_t u1, uint64_t *sum, uint32_t *min_count, uint32_t *max_count,
                          uint8_t *miss);
/* CCDBG::readCov(string, low, up, colour) (src/CCDBG.cpp:89-122) for every (string, colour): low / up hold one
 * cutoff per colour; arrays are string-major: x[i * n_colors + c].  ok = 0 (and sum = 0) when a k-mer is
 * missing from colour c's database or a count lies outside (low[c], up[c]).  [host|dev] */
int pf_string_cov_colored(pf_ctx *, const char *text, const uint64_t *str_off, uint32_t n_str, const uint32_t *low,
                          const uint32_t *up, uint64_t *sum, uint8_t *ok);

/* ---- (e) one graph over the GPUs of a node: the exchange step -------------------------------------------------------------
 * the graph, the CSR and the count table are replicated in every GPU's HBM, every rank (one process per GPU) runs
 * findSuperBubble and the owner scan, and rank r aligns, formats and writes its contiguous slice of the bubble list.  What the ranks
 * must tell each other is small: how many bubbles each of them called (var_count numbers bubbles across the whole run, src/CDBG.cpp:
 * 1254-1258), then the sizes of their ten text slabs with their allele histograms and coverage counters -- two all-gathers of a few
 * 64-bit words, over RCCL (xGMI between the GPUs).  No payload crosses ranks.
 * pf_comm_unique_id: called by one rank, the 128 bytes reach the others by any means (the CLI: a socket pair made before fork);
 * pf_comm_init: every rank, on its context (= its GPU); collective.  librccl is loaded here, not at start-up.
 * pf_gather: all[r * n + i] = word i of rank r, n <= 64, host pointers; collective. */
#define PF_COMM_ID_BYTES 128
int pf_comm_unique_id(unsigned char id[PF_COMM_ID_BYTES]);
int pf_comm_init(pf_ctx *, const unsigned char id[PF_COMM_ID_BYTES], int rank, int world);
int pf_gather(pf_ctx *, const uint64_t *mine, uint32_t n, uint64_t *all);
void pf_comm_destroy(pf_ctx *);

/* ---- `PloidyFrost model`: the Gaussian-mixture fit of the allele frequencies (src/GmmModel.cpp, src/Main.cpp:636-692) ----
 * pf_gmm_upload keeps the values (GmmModel::allele_fre, after the reader's frequency filter) in HBM; pf_gmm_fit is
 * GmmModel::resize(gauss) + emIterate() (src/GmmModel.cpp:8-20, 371-385) on them: means fixed at i/(gauss+1), weights and
 * variances re-estimated until the log-likelihood gains at most max_delta or max_iter iterations ran, with emStep's weight
 * thresholds m_thre / n_thre (:318-330).  Outputs: gauss weights / means / variances, the log-likelihood (the sum, not the
 * average) and the number of iterations.  fp64; sums are tree-shaped (the reference's are sequential), same order every run. */
#define PF_GMM_MAX_GAUSS 16
int pf_gmm_upload(pf_ctx *, const double *values, uint64_t n);
uint64_t pf_gmm_count(const pf_ctx *);
int pf_gmm_fit(pf_ctx *, uint32_t gauss, double m_thre, double n_thre, int32_t max_iter, double max_delta, double *weights,
               double *means, double *vars, double *loglik, uint32_t *iterations);
/* The values pf_gmm_fit reads, copied to the host: the first min(cap, pf_gmm_count) of them. */
int pf_gmm_values(pf_ctx *, double *dst, uint64_t cap);
/* The Gaussian kernel density of the values pf_gmm_fit reads (csrc/pf_density.hip): the curve script/Drawfreq.R draws, by ggplot2's
 * geom_density defaults.  bandwidth = adjust * bw.nrd0: 0.9 * min(sd, IQR / 1.34) * n^(-1/5) with the two-pass sample standard
 * deviation (divisor n - 1) and type-7 quartiles; when that minimum is 0 the first non-zero of sd, |values[0]|, 1 takes its place.
 * Grid: `points` (PF_DENSITY_MIN_POINTS .. PF_DENSITY_MAX_POINTS) abscissae x[j] = min + j * (max - min) / (points - 1), the last
 * one max itself.  density[j] = 1 / (n * bw) * sum_i phi((x[j] - v[i]) / bw): the exact sum -- R's density() bins the values onto
 * 1024 cells and convolves by FFT, so its numbers differ by its binning error; parity with R is unpinned.  fp64; every sum has a
 * shape that depends on n and points only (no floating-point atomics), so two calls give the same bits.  The array is left as it
 * was: pf_gmm_fit and pf_call_model_color_select may precede or follow.  x and density: `points` doubles each; info: the record.
 * PF_ERR_ARG (pf_last_error): fewer than two values ("need at least 2 data points"), a value that is not finite (named with the
 * index of the first one), points or adjust out of range. */
#define PF_DENSITY_MIN_POINTS 2
#define PF_DENSITY_MAX_POINTS 4096
typedef struct pf_density_info {
    uint64_t n;
    double min, max, sd, q1, q3, bw;
    double order[4]; /* x(lo), x(lo+1) of Q(0.25), then of Q(0.75) */
} pf_density_info;
int pf_gmm_density(pf_ctx *, uint32_t points, double adjust, double *x, double *density, pf_density_info *info);

/* ---- the model fed from the resident call streams (csrc/pf_call_model.hip) ----
 * The values `PloidyFrost model` reads back from <outpre>_bicov / _tricov / _tetracov.txt (-f) or <outpre>_allele_frequency.txt (-g)
 * are defined by the TEXT of those files; K-TEXT leaves that text in HBM piece by piece.  These three calls turn it into the array
 * pf_gmm_fit reads without a file, a host loop or a second context, element for element what GmmModel::readCovFile / readFreFile
 * (csrc/host/pf_gmm_model.cpp, reference src/GmmModel.cpp:21-257) make of the files -- quirks included: atoi on "%g" fields, the
 * integer frequency test, the neighbour-pair "min", pentacov never read, the last frequency token counted twice.  The per-row rule
 * is csrc/pf_model_rows.hpp, shared with the host (pfh_model_rows).  Single-sample path; the colored one behind
 * pf_call_model_filter_multi (below).
 *   pf_call_model_begin   source PF_MODEL_COV | PF_MODEL_FRE, minimum frequency q (`model -q`); drops the context's GMM array.
 *   pf_call_model_take    the piece in `slab`: after the pf_call_text / pf_call_text_range(_lane) call that made it, before the next
 *                         call that writes that slab (which then waits on the device until these kernels have read it).  Pieces
 *                         are taken in file order, from one thread.  Reads the text as K-TEXT wrote it, so
 *                         pf_call_set_numeric_packed / pf_call_set_alignseq_packed change nothing.  No wait, no copy to the host.
 *   pf_call_model_finish  waits; bi | tri | tetra (or the frequencies) end to end where pf_gmm_fit reads them, *n_values =
 *                         pf_gmm_count.  PF_ERR_ARG with pf_last_error naming stream and row (from 1, over the whole run) when a
 *                         coverage row sums to 0 (the reference divides by it) or a frequency row is not one number operator>>
 *                         reads ("nan", "inf") -- the errors the `model` sub-command gives -- or is a number the device cannot
 *                         convert exactly with one fp64 operation (more than 15 digits, decimal exponent beyond 22; "%g" never
 *                         prints such a frequency). */
enum pf_model_source { PF_MODEL_COV = 0, PF_MODEL_FRE = 1 };
int pf_call_model_begin(pf_ctx *, int source, double q);
int pf_call_model_take(pf_ctx *, int slab);
int pf_call_model_finish(pf_ctx *, uint64_t *n_values);
/* ---- a row filter in front of the model (csrc/pf_filter_rows.hpp) ----
 * The options of `ploidyfrost filter` (script/Filter.R; csrc/host/pf_filter.hpp FilterOptions) without the prefixes.  With a filter
 * the collection reads the four coverage streams (_bicov, _tricov, _tetracov, _pentacov) for either source and gives the array
 * that `filter` followed by `model -f` (cov) / `model -g <filtered>_allele_frequency.txt` (fre) would read, without writing a
 * filtered table: for fre the kept rows' frequencies column by column (all A-frequencies of the bi rows, all B-frequencies, ...,
 * 14 columns), each in (frequency, 1 - frequency), rounded to 7 places as R rounds and prints them, the last one counted twice.
 *   pf_call_model_filter     between pf_call_model_begin and the first take; NULL = no filter (the state after begin).
 *   pf_call_model_take_text  a piece of the text of stream `stream_ord` of the collection (without a filter: cov 0..2 = bi, tri,
 *                            tetra, fre 0; with one: 0..3 = bi, tri, tetra, penta) from host memory through the same kernels:
 *                            upload, then the collection's launches.  Pieces of a stream in file order, cut behind line feeds.
 * pf_call_model_finish then also refuses, naming stream and row: a row without its A + 5 fields or with a cell that is no finite
 * decimal number (what the host filter refuses), a kept coverage R would print in scientific notation (source cov; the
 * three-command chain handles those), and -- R's own error, the calling files being complete -- four tables that keep no row. */
typedef struct pf_filter_opts {
    int simple, indel, snp;          /* -S, -I, -P */
    long long low, up;               /* -l, -u   every coverage in (low, up) */
    long long num, distance, size;   /* -n VarNum < num, -d VarDis > distance, -s VarType < size */
    double frequency;                /* -q       frequencies in (q, 1 - q) */
} pf_filter_opts;
int pf_call_model_filter(pf_ctx *, const pf_filter_opts *);
int pf_call_model_take_text(pf_ctx *, int stream_ord, const char *host_text, uint64_t len);
/* ---- the multi form: the colored tables behind `ploidyfrost filter-multi`'s predicates ----
 * The colored path writes rows of A + 7 fields (A coverages, colour, isStrict, VarType, VarId, VarNum, Cramer's V, VarDis); the rule
 * is the opt.multi branch of run_filter (csrc/host/pf_filter.cpp) in csrc/pf_filter_rows.hpp: the predicates of the single-sample
 * filter without the clause on the sum of the first four coverages, Cramer's V > cramer (strictly), colour == color when color >= 0.
 * Behind it nothing changes: the array is what `filter-multi` followed by `model -f` / `model -g` reads.
 *   pf_call_model_filter_multi  between pf_call_model_begin and the first take, instead of pf_call_model_filter.  each_color = 0:
 *                               one collection, of colour `color` or pooled (color < 0).  each_color != 0 (with color < 0 only): the
 *                               pooled collection, each value with its row's colour beside it; pf_call_model_finish then gives the
 *                               pooled array and count and keeps the tokens for pf_call_model_color_select.  NULL: no filter.
 *   pf_call_model_color_count   after such a finish: one more than the largest colour that kept a row (0: none, or no such finish).
 *   pf_call_model_color_select  makes the array of colour `color` -- what the chain run with -c color reads, element for element --
 *                               the context's GMM array (pf_gmm_fit, pf_gmm_values), *n_values its length; a colour that kept no
 *                               row: PF_OK, *n_values = PF_MODEL_NO_ROW and the array as it was.  *n_values = 0: rows kept that
 *                               hold no value (cov: penta rows alone; fre: all outside the model's test) -- nothing to fit.
 *                               Any number of times, any order.
 * Refusals (PF_ERR_ARG, pf_last_error): pf_call_model_filter_multi outside begin .. first take, with frequency > 0.5, with
 * each_color and color >= 0 or without options; pf_call_model_take on a colored context without the multi filter (the tables have
 * other columns) and with it on a single-sample one; pf_call_model_filter on a colored context; pf_call_model_color_select
 * without a finished each_color collection or with a colour outside 0 .. PF_MAX_COLORS - 1.  pf_call_model_finish refuses as with
 * pf_call_model_filter (a row without its A + 7 fields is R's "did not have <table + 9> elements"; a Cramer's V of 0 / 0, printed
 * "-nan", is a cell that is no finite decimal number) and, split by colour, a kept row whose colour cell is no integer in
 * 0 .. PF_MAX_COLORS - 1; a refusal the model gives for a kept row (a sum of 0, scientific notation) then refuses every colour,
 * as it refuses the pooled collection. */
typedef struct pf_filter_multi_opts {
    int simple, indel, snp;
    long long low, up;
    long long num, distance, size;
    double frequency;
    long long color;                 /* -c       rows of this colour; < 0: every colour */
    double cramer;                   /* -v       Cramer's V > cramer */
} pf_filter_multi_opts;
#define PF_MODEL_NO_ROW 0xFFFFFFFFFFFFFFFFull
int pf_call_model_filter_multi(pf_ctx *, const pf_filter_multi_opts *, int each_color);
uint32_t pf_call_model_color_count(const pf_ctx *);
int pf_call_model_color_select(pf_ctx *, int color, uint64_t *n_values);
/* Bytes of the ten result streams the pf_call_fetch* calls of this context have copied to the host so far. */
uint64_t pf_call_fetched_bytes(const pf_ctx *);

/* ---- pinned host memory for the exchange buffers (optional: pageable memory works, slower) ---- */
int pf_host_alloc(pf_ctx *, size_t bytes, void **out);
/* bytes from device memory to (pinned) host memory, synchronous: for callers that hold device pointers but no HIP runtime */
int pf_fetch(pf_ctx *, void *dst_host, const void *src_dev, uint64_t bytes);
void pf_host_free(pf_ctx *, void *p);

/* ---- self tests ---------------------------------------------------------------------------- */
/* The prefix sums and the flag selection the library runs between its kernels (csrc/pf_scan.hpp), over n pseudo-random elements
 * against sequential host arithmetic: PF_OK, or PF_ERR_HIP with the first difference in pf_last_error. */
int pf_selftest_scan(pf_ctx *, uint64_t n, uint32_t seed);

/* ---- introspection ---------------------------------------------------------------------- */
int pf_device_name(pf_ctx *, char *buf, size_t cap);
/* "domain:bus:device.function" of the context's GPU (the host layer looks up its NUMA node with it) */
int pf_device_pci_bus_id(pf_ctx *, char *buf, size_t cap);
uint64_t pf_table_capacity(const pf_ctx *);
uint64_t pf_num_kmers(const pf_ctx *);

#ifdef __cplusplus
}
#endif
#endif /* PLOIDYFROST_HIP_H_ */
