// `ploidyfrost mask`: the host side of K-MASK (pf_mask_reads / pf_mask_fastq in ploidyfrost_hip.h, the rule in ../pf_mask_rule.hpp) --
// `kmc_tools filter -hm <db> <reads.fq> -ci<L>` of the reference's workflow (README step 2, script/pipeline/3.filter) against a
// database that is decoded once and looked up in HBM.  (The host's plain restatement of the rule, pf_mask::mask_read and
// pf_mask::index_fastq, lives in the rule header itself.)
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "ploidyfrost_hip.h"

namespace pfh {

struct CountOptions;   // pf_count_host.hpp

struct MaskTimes {
    double load_s = 0;     // database: map, decode, histogram, table (with -k: the count of the inputs instead)
    double stream_s = 0;   // first byte read to last byte written (wall)
    double device_s = 0;   // of it: inside pf_mask_fastq (upload, kernels, download)
    double read_s = 0;     // of it, beside the device: read() of the inputs
    double write_s = 0;    // of it, beside the device: write() of the output
};

// Masks the inputs, one after the other, into out_path (written under a temporary name, renamed at the end; nothing is left under
// either name after a refusal).  auto_lower: low = max(10, cutoffL) of the database's own histogram (K-HIST), as `cutoffL -d` prints
// it.  chunk_bytes = 0: MASK_DEFAULT_CHUNK (pf_reads_stream.hpp).  0 = ok, else worded in err (format refusals name the input and the 1-based record).
// gz_out (`--gz-out`): out_path is blocked gzip, deflated on the device behind K-MASK (GzOutFile, pf_gz_out_host.hpp).
int mask_fastq(const std::string &db_prefix, const std::vector<std::string> &inputs, const std::string &out_path, uint32_t low, uint32_t up,
               bool auto_lower, uint64_t chunk_bytes, int device, pf_mask_stats &stats, uint32_t &lower_used, MaskTimes *times, std::string &err,
               bool gz_out = false);
// The same without a database (`mask -k`): the inputs are counted first (K-COUNT, pf_count_host.hpp), the finished counters give the
// histogram and the table, and the inputs are streamed a second time through K-MASK -- what `count ... -o db` followed by
// `mask -d db ...` gives.  db_out (may be empty): the database is written as well.
int mask_fastq_counted(const CountOptions &count, const std::string &db_out, const std::vector<std::string> &inputs, const std::string &out_path,
                       uint32_t low, uint32_t up, bool auto_lower, uint64_t chunk_bytes, int device, pf_mask_stats &stats, uint32_t &lower_used,
                       MaskTimes *times, std::string &err, bool gz_out = false);

}  // namespace pfh
