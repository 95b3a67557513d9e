// `ploidyfrost count`: the host side of K-COUNT (pf_count_* and pf_kmc_encode in ploidyfrost_hip.h, the rule in ../pf_count_rule.hpp)
// -- step `2.kmc_db` of the reference's workflow (`kmc -ci1 -cs10000 -k25 @FILES kmc_sample tmp`): the FASTQ inputs streamed through
// the count table in HBM over the reader and device threads of the reads stream (pf_reads_stream.hpp), the kept counters written as a KMC1
// database.  (The host's plain restatement of the rule, pf_count::count_reads_host and pf_count::encode_kmc1_host, lives in the rule
// header itself.)
#pragma once
#include <stdint.h>

#include <functional>
#include <string>
#include <vector>

#include "../pf_count_rule.hpp"
#include "pf_reads_stream.hpp"
#include "ploidyfrost_hip.h"

namespace pfh {

struct CountOptions {   // kmc's letters and defaults
    uint32_t k = 25;
    uint64_t ci = pf_count::DEFAULT_CI, cx = pf_count::DEFAULT_CX, cs = pf_count::DEFAULT_CS;
    bool both_strands = true;     // false: -b
    uint64_t chunk_bytes = 0;     // 0: MASK_DEFAULT_CHUNK
    uint64_t initial_slots = 0;   // 0: twice the first chunk's bytes
    std::string hist;             // --hist: the histogram file of the finished counters
    bool fasta = false;           // --fasta: a chunk whose first byte is '>' goes through pf_count_fasta (K-FASTA, ../pf_fasta_rule.hpp)
    int gz = 0;                   // --gz (1), --gz-plain (2: any gzip, K-GUNZIP): inputs with the gzip magic are blocked gzip, inflated on the device (pf_gz_host.hpp)
};
struct CountTimes {
    double stream_s = 0;   // first byte read to the last chunk counted (wall)
    double finish_s = 0;   // flag, compact, sort (and the histogram)
    double write_s = 0;    // encode, download, the two files
};
struct Counted {   // what pf_count_finish gives: device arrays for pf_count_histogram, pf_upload_counts, pf_kmc_encode
    uint64_t *kmers = nullptr;
    uint32_t *counts = nullptr;
    uint64_t n = 0;
};

// the refusal of the options (pf_count::CutClause, 0 = none): k, ci < 1, ci > cx, cs < 1, a value above 2^32 - 1; writes: a database
// is written (k >= 5)
int count_options_clause(const CountOptions &opt, bool writes);
// begin, the inputs (as the preflight left them) through pf_count_fastq / pf_count_fasta, finish.  `who` words the refusals ("count", "mask").  0 = ok (the caller frees `out` with
// pf_device_free), else worded in err; no count is left open.
int count_stream(pf_ctx *ctx, const char *who, const std::vector<ReadsInput> &inputs, const CountOptions &opt, Counted &out, pf_count_stats &stats,
                 CountTimes &tm, std::string &err);
// the same around any pass that feeds the open count (`run STEP...`: the raw reads through the trimmed entry points): pf_count_begin,
// pass(err) (0 = ok, else err is worded and the count is aborted), pf_count_finish
int count_stream_with(pf_ctx *ctx, const char *who, const CountOptions &opt, const std::function<int(std::string &)> &pass, Counted &out,
                      pf_count_stats &stats, CountTimes &tm, std::string &err);
// the rows of the histogram of the finished counters, as pfh::kmc_rows gives them for the written database.  PF_OK, else pf_last_error
int counted_rows(pf_ctx *ctx, const Counted &db, const CountOptions &opt, std::vector<uint64_t> &rows);
// <prefix>.kmc_pre / <prefix>.kmc_suf from the finished counters: encoded on the device block by block, written under temporary
// names and renamed at the end; nothing is left under any of the four names after a refusal
int write_counted(pf_ctx *ctx, const char *who, const std::string &prefix, const Counted &db, const CountOptions &opt, std::string &err);
// the whole of `ploidyfrost count`.  FASTA, gzip (with opt.gz: gzip that is not blocked gzip) and an output that is an input are refused before a device context exists
int count_fastq(const std::vector<std::string> &inputs, const std::string &out_prefix, const CountOptions &opt, int device, pf_count_stats &stats,
                CountTimes *times, std::string &err);

}  // namespace pfh
