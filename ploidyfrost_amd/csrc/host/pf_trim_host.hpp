// `ploidyfrost trim`: the host side of K-TRIM (pf_trim_fastq / pf_trim_fastq_pair in ploidyfrost_hip.h, the rule in ../pf_trim_rule.hpp) --
// `trimmomatic SE|PE -phred33 ... LEADING:10 TRAILING:10 SLIDINGWINDOW:3:20 MINLEN:50` of the reference's workflow
// (script/pipeline/1.trim).  (The host's plain restatement of the rule, pf_trim::trim_read and pf_trim::trim_fastq, lives in the rule
// header itself.)
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "pf_clip_host.hpp"
#include "pf_dedup_host.hpp"
#include "pf_qc_host.hpp"
#include "ploidyfrost_hip.h"

namespace pfh {

struct TrimOptions {
    std::vector<pf_trim_step> steps;
    uint32_t phred = 33;
    std::string trimlog;        // "" = none
    uint64_t chunk_bytes = 0;   // 0 = MASK_DEFAULT_CHUNK (pf_reads_stream.hpp)
    bool gz_out = false;        // --gz-out: every read output is blocked gzip, deflated on the device behind the step (GzOutFile, pf_gz_out_host.hpp)
    ClipOptions clip;           // --adapters: K-CLIP in front of the steps; no step is needed beside it
    std::string report;         // --report: "" = none; K-QC adds both stages of every chunk to a report (pf_qc_host.hpp), written beside the other outputs
    DedupOptions dedup;         // --dedup: K-DEDUP behind the steps drops every later copy of a kept unit; no step is needed beside it
    int gz = 0;                 // --gz (1), --gz-plain (2: any gzip, K-GUNZIP): inputs with the gzip magic are blocked gzip, inflated on the device (pf_gz_host.hpp)
};
struct TrimTimes {
    double stream_s = 0;   // first byte read to last byte written (wall)
    double device_s = 0;   // of it: inside pf_trim_fastq / pf_trim_fastq_pair (upload, kernels, download)
    double read_s = 0;     // of it, beside the device: read() of the inputs
    double write_s = 0;    // of it, beside the device: write() of the outputs
};

// The refusals of the steps and the offset (and of the clip's seed and score), worded as the sub-command words them (0 = none).
int trim_options_clause(const TrimOptions &opt, std::string &err);

// Single-ended: the inputs, one after the other, through K-TRIM into out_path; opt.trimlog gets one line per record,
// `<header without '@'> <kept length> <b> <e> <n - e>` (a dropped record: 0 0 0 0).  Every output is written under a temporary name
// and renamed at the end; nothing is left under any name after a refusal.  0 = ok, else worded in err (format refusals name the
// input and the 1-based record).  With opt.clip the adapter file is read and refused before a device context exists, every read is
// clipped first (the log's e is then counted from the clipped read) and *clip (may be null) reports it.  With opt.report the
// report of both stages is written to that path as every other output is, and *qc (may be null) holds its tables.  With opt.dedup
// one table lives over the whole stream (all inputs together), a dropped duplicate is logged as `0 0 0 0`, and *dedup (may be
// null) holds the statistics.
int trim_fastq(const std::vector<std::string> &inputs, const std::string &out_path, const TrimOptions &opt, int device, pf_trim_stats &stats,
               TrimTimes *times, std::string &err, ClipReport *clip = nullptr, QcReport *qc = nullptr, pf_dedup_stats *dedup = nullptr);
// Paired: record r of in1 pairs with record r of in2; out_paths = o1 u1 o2 u2 (both kept / file 1 alone / both kept / file 2 alone).
// The lock-step stream of pf_reads_stream.hpp (two reader threads, one device stage, each file its own carry), a writer per output.  A file that ends while the other still
// holds a whole record is refused by name.  The trimlog has record r of file 1, then record r of file 2.
int trim_fastq_pair(const std::string &in1, const std::string &in2, const std::string out_paths[4], const TrimOptions &opt, int device,
                    pf_trim_stats stats[2], TrimTimes *times, std::string &err, ClipReport *clip = nullptr, QcReport *qc = nullptr,
                    pf_dedup_stats *dedup = nullptr);

}  // namespace pfh
