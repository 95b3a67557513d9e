// pfh::CDBG -- the product's host-side mirror of the reference class CDBG
// (reference src/CDBG.hpp:20-41, driven from src/Main.cpp:829-849):
//
//     CDBG g(graph, z, M, D, G, kmc_prefix);
//     g.setUnitigId(outpre, graphfile, threads);
//     g.printInfo(verbose, outpre);                              // only with -i
//     g.findSuperBubble_multithread_ptr(outpre, threads);
//     g.ploidyEstimation_multithread_ptr(outpre, lower, upper, threads);
//
// Same method names, argument meaning, output files (./PloidyFrost_output/<outpre>_*.txt) and
// stdout lines.  Differences, all deliberate:
//   * every compute-heavy step runs on the MI355X through include/ploidyfrost_hip.h
//     (adjacency join, superbubble traversals, per-unitig and per-string k-mer coverage,
//     Needleman-Wunsch fill + traceback); the host keeps only the order-dependent state
//     replay, the progressive-alignment bookkeeping and the text formatting;
//   * methods return an int status instead of calling exit(); main() turns a failure into the
//     reference's "message + exit(EXIT_FAILURE)";
//   * output is always the deterministic `-t 1` ordering, whatever `threads` says.
#pragma once
#include <chrono>
#include <memory>
#include <condition_variable>
#include <mutex>

#include "pf_bfs_host.hpp"
#include <cstdint>
#include <memory>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "pf_gmm_model.hpp"
#include "pf_host_colors.hpp"
#include "pf_host_graph.hpp"
#include "pf_pinned.hpp"
#include "pf_replay_par.hpp"
#include "pf_state.hpp"
#include "ploidyfrost_hip.h"

namespace pfh {

struct Scoring {
    double match = 2, mismatch = -1, gap = -3;
};

struct PhaseTimes {
    double bfs_device_s = 0, replay_s = 0, bubble_write_s = 0;
    double cov_device_s = 0, tasks_s = 0, align_s = 0, sites_s = 0, format_s = 0, write_s = 0;
    double find_total_s = 0, ploidy_total_s = 0;
    double scan_s = 0, scan_serial_s = 0, align_build_s = 0, align_device_s = 0, align_post_s = 0, align_choose_s = 0;
    uint64_t bfs_large = 0, bfs_large_seen = 0, bfs_max_seen = 0;  // traversals beyond 4096 unitigs
    uint64_t bfs_large_used = 0, bfs_large_used_max = 0;            // ... that the replay's gate let through, and the longest of those
    uint64_t candidates = 0, bfs_deferred = 0, bubbles_out = 0, tasks = 0, align_jobs = 0, site_strings = 0;
    uint64_t host_commit_records = 0, host_walk_vertices = 0;   // findSuperBubble's host share: records committed on a host thread (large components + walked traversals), vertices the walkers visited
    uint64_t snp_jobs = 0, pair_jobs = 0, wave_jobs = 0, stack_jobs = 0;   // of align_jobs: by K-SNP, by K-PAIR, by K-BUBBLE, by K-STACK
};

// The count database on its way to HBM while the caller is still reading the graph file: context creation, header / prefix
// table parse, K-KMC decode and the table build need nothing from the graph, so a front end starts them first
// (CountsLoader::start) and hands the loader to the CDBG constructor, which waits for it and adopts its context.
struct CountsLoader {
    ~CountsLoader();
    void start(int device, const std::string &kmc_prefix);
    // Instead of start(): a context that holds the count table already (`ploidyfrost run`: pf_upload_counts of the counters it has
    // just counted), with the histogram rows of those counters (pfh::counted_rows) for the thresholds.  No thread, no file; the
    // loader owns the context from here, as after start().
    void adopt(pf_ctx *c, int k_, bool both_strands_, std::vector<uint64_t> rows_, uint64_t rows_min_count_);
    // valid after wait()
    pf_ctx *ctx = nullptr;
    int status = 0;
    std::string error;
    bool both_strands = true;
    int k = 0;
    // set before start(): the rows of the database's k-mer histogram (pf_cutoffs.hpp) are counted from the decoded counters before
    // they are freed (K-HIST); off: nothing more is launched or allocated
    bool want_rows = false;
    std::vector<uint64_t> rows;
    uint64_t rows_min_count = 0;
    void wait() { if (th_.joinable()) th_.join(); }
    pf_ctx *release() { pf_ctx *c = ctx; ctx = nullptr; return c; }
    // the context as soon as it exists (the count table is still on its way): nullptr when its creation failed.  Only calls
    // that are safe beside the table's ingest may use it before wait() (pf_gfa_parse).
    pf_ctx *wait_context() {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return ctx_known_; });
        return ctx;
    }

private:
    std::thread th_;
    std::mutex mu_;
    std::condition_variable cv_;
    bool ctx_known_ = false;
};

struct FindTrace;   // pf_cdbg_impl.hpp

class CDBG {
public:
    CDBG(UnitigSet &graph, const size_t &complexsize, double &m, double &d, double &g, std::string kmc_db = "",
         int device = 0, bool quiet = false, CountsLoader *counts = nullptr);
    virtual ~CDBG();
    CDBG(const CDBG &) = delete;
    CDBG &operator=(const CDBG &) = delete;

    bool good() const { return status_ == 0; }
    int status() const { return status_; }
    const std::string &error() const { return err_; }

    int setUnitigId(const std::string &outpre, const std::string &graphfile, const size_t &thr);
    int printInfo(const bool &verbose, const std::string &outpre);
    int findSuperBubble_multithread_ptr(const std::string &outpre, const size_t &thread);
    int ploidyEstimation_multithread_ptr(const std::string &outpre, const int &lower, const int &upper, const size_t &thr);

    // extras (not in the reference interface)
    void set_output_dir(const std::string &dir) { outdir_ = dir; }  // default "PloidyFrost_output"
    void set_quiet(bool q) { quiet_ = q; }
    void set_threads(unsigned t) { threads_ = t; }                  // host threads; 0 = use the `thr` argument
    void set_third_tier_on_host(bool on) { third_tier_on_host_ = on; }   // default on; off = one wavefront per giant traversal
    void set_write_files(bool w) { write_files_ = w; }              // bench: format but do not touch the disk
    void set_batch_bubbles(size_t n) { batch_bubbles_ = n; }
    // resident pipeline: text pieces (4 x batch_bubbles bubbles each) per alignment launch; default 64: a whole pass of up
    // to 2^24 bubbles is aligned in one launch sequence
    void set_align_pieces(size_t n) { align_pieces_ = n ? n : 1; }
    // write <outpre>_super_bubble.txt in the background while PloidyEstimation runs (complete when that call, the next
    // findSuperBubble or the destructor returns); off by default: the file is complete when findSuperBubble returns
    void set_overlap_output(bool on) { overlap_output_ = on; }
    // PloidyEstimation through the device's resident calling pipeline (pf_call_*, the default for the single-sample path) or,
    // off, through the host-threaded pipeline around pf_align_bubbles / pf_string_cov (what the colored path uses)
    void set_resident_calling(bool on) { resident_ = on; }
    // Text format of the reference's `-t N` run with N > 1 (single-sample path): BubbleId / var_count from 0, the allele_frequency
    // rows of a bubble grouped by arity (src/CDBG.cpp:1829, 2056, 2158-2162, 2550) and its stdout wording; the order of rows
    // stays the deterministic `-t 1` one (the reference's own depends on thread timing).
    int set_reference_threads(size_t n);
    // The ploidy estimate in the same run (single-sample path, resident pipeline): PloidyEstimation hands every text piece to
    // pf_call_model_take while it is resident, then fits on the same device context (run_model over a GmmModel that borrows it) and
    // writes <outpre>_model_result.txt -- what `model -f <outpre>` (source cov) / `model -g <outpre>_allele_frequency.txt` (fre)
    // writes from the files.  only: none of the ten calling files is written and their text never leaves the device.
    struct ModelOptions {
        bool on = false, only = false;
        int source = 0;          // pf_model_source
        double q = 0;            // `model -q`
        int lo = 1, hi = 9;      // Gaussians, i.e. ploidy 2 .. 10 (`model -l / -u`)
        double m_thre = 5.0, n_thre = 2.0, max_delta = 0.01;
        int max_iter = 1000;
    };
    int set_model(const ModelOptions &o);
    // The kernel density of the array every fit of that model reads (pf_gmm_density), taken right after the fit: the pooled array,
    // and with each_color every colour's after its selection; written to <outpre>_allele_frequency_density.txt /
    // <outpre>_color<c>_allele_frequency_density.txt beside the model results.  After set_model; points == 0: off (as switching the
    // model off does).  An array of fewer than two values: the pass ends with "need at least 2 data points" once everything else is
    // complete; split by colour such a colour is listed (model_colors_without_density), gets no file, and the pass fails only when
    // no colour has a curve.
    int set_density(unsigned points, double adjust);
    const Density *model_density() const { return density_done_ ? &density_ : nullptr; }
    const std::vector<int> &model_colors_without_density() const { return color_no_density_; }
    // `ploidyfrost filter`'s row predicates in front of that model (pf_call_model_filter; the rule is csrc/pf_filter_rows.hpp): the
    // estimate of `filter` + `model` on this run's files, no filtered table written.  Null: no filter.  Refused unless a model is set;
    // switching the model off drops it.
    int set_filter(const pf_filter_opts *o);
    // the colored path: `ploidyfrost filter-multi`'s predicates (pf_call_model_filter_multi) in front of the model, which the colored
    // run accepts behind them only (its unfiltered tables pool every sample): set_model, then this, then PloidyEstimation.
    // each_color: one fit per colour that keeps a row, <outpre>_color<c>_model_result.txt each (needs color < 0).  Null: off.
    int set_filter_multi(const pf_filter_multi_opts *o, bool each_color);
    // of the last PloidyEstimation split by colour, in colour order: the fits as model_fits() has them, the values copied from the
    // device, the colours below model_color_count() that kept no row, and those that kept rows which hold no value for the model
    // (cov: penta rows alone; fre: every frequency outside the model's test) -- neither kind is fitted or gets a file
    struct ColorFit {
        int color = 0;
        std::vector<GmmModel::Fit> fits;
        double ploidy = 0;
        std::vector<double> values;
        bool has_density = false;
        Density density;
    };
    const std::vector<ColorFit> &model_color_fits() const { return color_fits_; }
    const std::vector<int> &model_colors_without_rows() const { return color_none_; }
    const std::vector<int> &model_colors_without_values() const { return color_empty_; }
    const std::vector<double> &model_pooled_values() const { return pooled_values_; }
    bool model_was_each_color() const { return last_each_; }   // of the last pass, not of the settings
    // of the last PloidyEstimation with a model: one record per number of Gaussians, the value of the result file's last line and
    // that line; how many values the device array holds
    const std::vector<GmmModel::Fit> &model_fits() const { return model_fits_; }
    double model_ploidy() const { return model_ploidy_; }
    const std::string &model_last_line() const { return model_last_line_; }
    uint64_t model_count() const { return model_n_; }
    // bytes of the ten calling streams the last PloidyEstimation copied from the device (0 with ModelOptions::only)
    uint64_t text_bytes_fetched() const { return text_fetched_; }
    // ---- one graph over several GPUs (reference owner rule src/CDBG.cpp:1190, 1352, 1656-1679) -------------
    // findSuperBubble: every rank traverses the entrances of its unitig range (find_shard), the ranks exchange the records,
    // every rank replays all of them (find_replay; rank 0 writes the file).  PloidyEstimation: the scan and the sequential pass
    // run on every rank (ploidy_select), each rank aligns its slice of the bubble list (ploidy_align), the ranks exchange how
    // many of their bubbles were called, format with that base (ploidy_text) and, knowing every rank's slab sizes, write
    // their slabs at their offsets of the shared result files (ploidy_write).
    int find_shard(uint32_t u0, uint32_t u1);
    const std::vector<pf_bfs_record> &shard_records() const { return shard_rec_; }
    const std::vector<uint32_t> &shard_pool() const { return shard_pool_; }
    // dev_records / dev_pools (optional): the same shards where they already lie in device memory (after an all-gather), so that
    // the components of the parallel replay are found without another upload; pool_lens = entries of each pool
    int find_replay(const std::string &outpre, uint32_t n_shards, const pf_bfs_record *const *records, const uint64_t *n_records,
                    const uint32_t *const *pools, bool write_file, const uint64_t *pool_lens = nullptr,
                    const pf_bfs_record *const *dev_records = nullptr, const uint32_t *const *dev_pools = nullptr);
    // the commit replay on host threads (pf_replay_par.hpp): 0 = sequential; default min(threads, 32) for the single-sample path
    void set_replay_threads(int t) { replay_threads_ = t; }
    // one graph on several ranks with findSuperBubble run by each of them: only one rank writes <outpre>_super_bubble.txt
    void set_write_super_bubble(bool on) { write_sb_ = on; }
    int ploidy_select(int lower, int upper, uint64_t &n_bubbles);
    int ploidy_select(const std::vector<std::pair<int, int>> &cutoff, uint64_t &n_bubbles);   // colored: one pair per colour
    int ploidy_align(uint64_t t0, uint64_t t1, uint64_t &n_called);
    int ploidy_text(uint64_t var_count_base, uint64_t sizes[PF_CALL_STREAMS], uint64_t counters[8]);
    int ploidy_write(const std::string &outpre, const uint64_t offsets[PF_CALL_STREAMS], const uint64_t totals[PF_CALL_STREAMS], bool truncate);
    pf_ctx *device() { return ctx_; }
    const PhaseTimes &times() const { return times_; }
    uint64_t allele_sites(int arity) const { return allele_[arity - 2]; }
    uint64_t core_cov() const { return core_cov_; }
    uint64_t core_num() const { return core_num_; }
    uint64_t n_superbubbles() const { return n_super_bubble_; }
    // (after commits on the device the host copy is fetched when somebody asks)
    const std::vector<uint8_t> &state_flags() { sync_state_to_host(); return flags_; }
    const std::vector<uint32_t> &state_plus() { sync_state_to_host(); return plus_; }
    const std::vector<uint32_t> &state_minus() { sync_state_to_host(); return minus_; }
    int sync_state_to_host();
    uint64_t output_bytes() const { return out_bytes_; }
    // text of <outpre>_allele_frequency.txt of the last run (the record slab a multi-GPU job gathers)
    // (after a pass that wrote its files the rows are read back from <outpre>_allele_frequency.txt when somebody asks, instead of
    // being copied aside piece by piece under the writer of every pass)
    const std::string &last_allele_frequency() const;

protected:
    // graph + adjacency on the device, no count database yet (the colored subclass brings its own)
    struct NoCounts {};
    // adopt: a context that exists already (`ploidyfrost run-multi`); the CDBG owns it from here
    CDBG(UnitigSet &graph, const size_t &complexsize, double &m, double &d, double &g, int device, bool quiet, NoCounts, pf_ctx *adopt = nullptr);
    int init_device(int device, pf_ctx *adopt = nullptr, bool colored = false);
    void start_prealloc();  // the first launches' device buffers, on a helper thread (single-sample, resident pipeline)
    // the path proper; cutoff holds one (lower, upper) pair (single sample) or one per colour
    int ploidy_estimation(const std::string &outpre, const std::vector<std::pair<int, int>> &cutoff, const size_t &thr);
    // the same through pf_call_* (pf_cdbg_call.cpp); call_select = scan + the sequential pass of the driver loop
    int ploidy_estimation_resident(const std::string &outpre, const std::vector<std::pair<int, int>> &cutoff, const size_t &thr);
    int call_select(const std::vector<std::pair<int, int>> &cutoff, uint64_t &n_tasks);
    bool resident_path() const { return resident_ && (col_ == nullptr || colored_resident_); }
    // set by CCDBG: the colour sets of the graph's unitigs (reference src/CCDBG.cpp path) and the stdout tag
    const ColorSets *col_ = nullptr;
    const char *tag_ = "CDBG";

    struct Task;
    using clk_time = std::chrono::steady_clock::time_point;
    // timing_lines: the `Cpu time` / `Real time` pair of findSuperBubble's stdout goes first
    int finish_find(const std::string &outpre, const FindTrace &tr, bool write_file, bool timing_lines);
    std::vector<pf_bfs_record> shard_rec_;
    std::vector<uint32_t> shard_pool_;
    ModelOptions model_;
    unsigned density_points_ = 0;   // 0: no density
    double density_adjust_ = 1.0;
    Density density_;
    bool density_done_ = false;
    std::vector<int> color_no_density_;
    bool filter_on_ = false;
    pf_filter_opts filter_ = {};
    bool multi_on_ = false, multi_each_ = false;
    pf_filter_multi_opts multi_ = {};
    std::vector<ColorFit> color_fits_;
    std::vector<int> color_none_, color_empty_;
    std::vector<double> pooled_values_;
    bool last_each_ = false;   // the last PloidyEstimation's model was split by colour (whatever the settings are by now)
    std::vector<GmmModel::Fit> model_fits_;
    double model_ploidy_ = 0;
    std::string model_last_line_;
    uint64_t model_n_ = 0, text_fetched_ = 0;
    pf_call_result slice_res_ = {};
    uint64_t slice_nb_ = 0, slice_var_base_ = 0;   // ploidy_align's range and ploidy_text's numbering base, for ploidy_write's pieces
    int fail(int st, const std::string &msg);
    int join_pending_write();
    int join_pending_ids();
    // pinned exchange buffers of the first pass, allocated on a helper thread while the graph goes to the device (page-locking
    // a few hundred MB costs tens of milliseconds; sizes are estimates from the unitig count, the phases grow them if needed)
    std::thread prealloc_, prealloc_walkers_, prealloc_call_, prealloc_align_;
    void join_prealloc() {
        if (prealloc_.joinable()) prealloc_.join();
        if (prealloc_walkers_.joinable()) prealloc_walkers_.join();
        if (prealloc_call_.joinable()) prealloc_call_.join();
        if (prealloc_align_.joinable()) prealloc_align_.join();
    }
    std::thread pending_ids_;
    int pending_ids_rc_ = 0;
    uint64_t ids_bytes_ = 0;
    int launch_coverage();
    uint64_t find_passes_ = 0;
    bool cov_ready_ = false;  // the coverage arrays in bx_ are those of the current graph and count table
    std::string cov_err_;
    bool overlap_output_ = false;
    std::thread pending_write_;
    int pending_rc_ = 0;
    int ensure_dir();
    int write_file(const std::string &name, const std::string &data);
    int write_pieces(const std::string &name, const std::vector<const std::string *> &pieces, uint64_t &bytes) const;
    int write_many(const std::vector<std::pair<std::string, std::vector<const std::string *>>> &files, unsigned threads);
    void replay(const pf_bfs_record &r, const uint32_t *list) { st_.replay(r, list); }

    UnitigSet &g_;
    size_t complex_size_;
    Scoring sc_;
    std::string outdir_ = "PloidyFrost_output";
    pf_ctx *ctx_ = nullptr;
    int status_ = 0;
    std::string err_;
    bool quiet_ = false, write_files_ = true;
    bool both_strands_ = true;
    unsigned threads_ = 0;
    int replay_threads_ = -1;   // -1: default
    bool write_sb_ = true;
    // commits on the device (pf_replay_device): the host arrays are stale until sync_state_to_host; big_f2_ = the per-side flag
    // bytes of the few components committed on the host (kept all-zero between passes)
    bool state_host_stale_ = false;
    bool colours_on_device_ = false;   // colored path: pf_replay_set_colours succeeded
    bool colored_resident_ = false;    // colored path: pf_call_set_colours succeeded -- the calling phase runs on the resident pipeline
    std::vector<uint8_t> big_f2_;
    bool commits_on_device() const;
    ParallelReplay par_;
    unsigned replay_threads(size_t thr) const;
    size_t host_threads(size_t thr) const;     // set_threads, else the call's `thr` argument
    unsigned walk_threads(size_t thr) const;   // ... of which so many may walk long traversals side by side
    void set_record_stats(const ReplayStats &s);
    // the steps of findSuperBubble (pf_cdbg_find.cpp): with the commits on the device ...
    struct EarlyWalks; struct DeviceFind; struct SlicedFind;
    int find_superbubbles_device(const std::string &outpre, const size_t &thr);
    int traverse_resident(EarlyWalks &early, DeviceFind &df, const FindTrace &tr);
    void walk_remaining(EarlyWalks &early, DeviceFind &df, const FindTrace &tr, unsigned threads);
    void walked_into_candidate_order(DeviceFind &df);
    int commit_large_on_host(DeviceFind &df, const FindTrace &tr, unsigned threads);
    int patch_device_state(const std::vector<uint32_t> &sides, const FindTrace &tr, unsigned threads);
    // ... and with the commits on the host: the device thread's side of the sliced pass
    void traverse_slices(SlicedFind &sf, const FindTrace &tr);
    int traverse_slice(SlicedFind &sf, int i, const FindTrace &tr);
    void walk_long(const FindTrace &tr, bool say_start, uint32_t entrance, pf_bfs_record &r, std::vector<uint32_t> &out);
    template <class Call> int with_deferred(uint64_t &n_deferred, Call call);
    template <class ListOf> void replay_sequential(const pf_bfs_record *rec, uint64_t n, ListOf list_of, ReplayStats &stats);
    // third K-BFS tier (traversals beyond 4096 vertices) on host cores, pf_bfs_host.hpp; false = the device's k_bfs_huge
    bool third_tier_on_host_ = true;
    WalkerPool walkers_;
    std::vector<uint32_t> deferred_;   // record indices pf_bfs_candidates_split leaves to the host walkers
    std::vector<uint32_t> deferred_ent_;   // their entrances (pf_bfs_candidates_begin)
    // vertex lists of the records walked on the host (pf_bfs_record::pad_ == 1, list_off = index), per K-BFS slice: a slice's
    // lists are complete before its records are handed to the replay
    std::vector<std::vector<uint32_t>> huge_lists_[4];

    std::vector<uint32_t> succ_, pred_;  // host copy of the CSR, [2N][4]
    // MyUnitig state (reference src/MyUnitig.hpp), array-indexed, with the commits that mutate it (pf_state.hpp)
    UnitigState st_;
    std::vector<uint8_t> &flags_ = st_.flags;
    std::vector<uint32_t> &plus_ = st_.plus, &minus_ = st_.minus;  // 0 = NULL, id = u + 1

    // pinned exchange buffers of pf_align_bubbles, three sets: one per batch in flight (reused from pass to pass)
    struct AlignExchange {
        PinnedBuf<char> text, otext;
        PinnedBuf<pf_bubble_path> paths;
        PinnedBuf<pf_bubble_task> tasks;
        PinnedBuf<pf_bubble_result> res;
        PinnedBuf<pf_bubble_site> osites;
        PinnedBuf<uint8_t> ogroups;
        PinnedBuf<uint32_t> oilen;
        void release_all() {
            text.release(); otext.release(); paths.release(); tasks.release(); res.release(); osites.release();
            ogroups.release(); oilen.release();
        }
    } ax_[3];
    // (a text piece = four batches: 131 072 bubbles, 18 MB over PCIe at k = 25 -- pieces short enough that the last one's PCIe copy and file
    // copy, which nothing overlaps, stay small)
    size_t batch_bubbles_ = 32768, align_pieces_ = 64;   // (text pieces of 4 x 32768 bubbles: tools/ab_pass.py BATCH=n, profiles/r16_experiments.txt)
    // pinned buffers of the whole-graph device calls
    struct BubbleExchange {
        PinnedBuf<pf_bfs_record> bfs_rec;
        PinnedBuf<uint32_t> bfs_pool;
        PinnedBuf<uint32_t> bfs_order;   // parallel replay: record indices grouped by class (pf_replay_order)
        PinnedBuf<uint64_t> cov_sum;
        PinnedBuf<uint32_t> cov_min;
        PinnedBuf<uint8_t> cov_miss;
        PinnedBuf<uint32_t> cov_max;  // colored path: per (colour, unitig) arrays, colour-major
        void release_all() {
            cov_max.release();
            bfs_rec.release(); bfs_pool.release(); bfs_order.release(); cov_sum.release(); cov_min.release();
            cov_miss.release();
        }
    } bx_;
    // exchange buffers of the resident calling pipeline: side records down, selection up, text slabs down
    struct CallExchange {
        PinnedBuf<pf_call_side> sides;
        PinnedBuf<uint32_t> kept;
        PinnedBuf<char> slab[2];
        void release_all() { sides.release(); kept.release(); slab[0].release(); slab[1].release(); }
    } cx_;
    bool resident_ = true;
    bool mt_format_ = false;
    // the result files of the resident pipeline and super_bubble.txt, kept open and mapped between passes (pf_cdbg_impl.hpp)
    std::unique_ptr<struct MappedOut[]> out_maps_;
    bool state_on_device_ = false;   // pf_call_set_state holds the state findSuperBubble left (finish_find uploads it)
    PinnedBuf<char> sb_text_;        // text of super_bubble.txt on its way from the device to the file
    PhaseTimes times_;
    mutable std::string last_allfre_, last_allfre_file_;
    mutable uint64_t last_allfre_bytes_ = 0;
    uint64_t allele_[4] = {0, 0, 0, 0};
    uint64_t core_cov_ = 0, core_num_ = 0, n_super_bubble_ = 0, out_bytes_ = 0;
};

// pfh::ColoredUnitigSet -- what the colored path needs of the reference's ColoredCDBG<MyUnitig>
// (bifrost/src/ColoredCDBG.hpp): the unitigs of the GFA file and their colour sets from the .bfg_colors file.
struct ColoredUnitigSet {
    UnitigSet graph;
    ColorSets colors;
    std::string err;
    // ColoredCDBG::read(graphfile, colorfile, nb_threads, verbose) (bifrost/src/ColoredCDBG.tcc:428-600)
    bool read(const std::string &graphfile, const std::string &colorfile, size_t nb_threads = 1, bool verbose = false);
    size_t getNbColors() const { return colors.n_colors; }
    int getK() const { return graph.k; }
    size_t size() const { return graph.n(); }
    // The same for a graph and a colour file that lie in memory (`ploidyfrost run-multi`): the GFA text as UnitigSet::open_gfa_memory
    // takes it (K-GFA reads the DA tags with the segments), the bytes of the colour file as pf_bfg::write laid them out.  Both stay the
    // caller's and outlive the set.  The colour sets are read by the CCDBG constructor once the device has parsed the segments
    // (colors_pending): the reader asks for every unitig's length, head k-mer and DA tag.
    bool open_memory(const char *host_text, uint64_t n, const char *device_text, const uint8_t *color_bytes, uint64_t n_color_bytes, size_t nb_threads = 1);
    bool colors_pending() const { return colors_pending_; }
    bool reload_colors();   // after the unitig order changed (abundant k-mers found by the device census), or the first time behind open_memory

private:
    std::string colorfile_;
    const uint8_t *color_bytes_ = nullptr;
    uint64_t n_color_bytes_ = 0;
    bool colors_pending_ = false;
    unsigned color_threads_ = 1;
};

// The count databases of a coloured run where they lie on the device already (`ploidyfrost run-multi`: every sample's finished
// counters), instead of a list of database names: per colour the k-mers, the counters and how many, with the filters every database
// would carry in its header.  The arrays stay the caller's; the context is adopted (CountsLoader::adopt's coloured twin).
struct ColorCounts {
    pf_ctx *ctx = nullptr;
    std::vector<const uint64_t *> kmers;
    std::vector<const uint32_t *> counts;
    std::vector<uint64_t> n;
    uint64_t min_count = 1, max_count = 0xFFFFFFFFull;
    int k = 0;
};

// pfh::CCDBG -- mirror of the reference class CCDBG (src/CCDBG.hpp:18-40, driven from src/Main.cpp:775-810):
//
//     CCDBG g(cdbg, z, M, D, G, kmc_list_file, threads);
//     g.setUnitigId(outpre, graphfile, threads);
//     g.findSuperBubble_multithread_ptr(outpre, threads);
//     g.ploidyEstimation_multithread_ptr(outpre, cutoffs, threads);      // one (lower, upper) per colour
//
// Output files are byte-identical to the reference's `-t 1` run.  All colours' count databases live in one
// HBM table (include/ploidyfrost_hip.h, pf_upload_counts_colored).
class CCDBG : public CDBG {
public:
    // rows_out: the rows of every database's k-mer histogram (pf_cutoffs.hpp), one vector per colour, counted from the decoded
    // counters of each (K-HIST); null: nothing more is launched or allocated
    CCDBG(ColoredUnitigSet &graph, const size_t &complexsize, double &m, double &d, double &g, std::string kmc_db_list = "",
          const size_t &thread = 1, int device = 0, bool quiet = false, std::vector<std::vector<uint64_t>> *rows_out = nullptr);
    // the adopting route: graph and colours through ColoredUnitigSet::open_memory, the joined table from device arrays
    CCDBG(ColoredUnitigSet &graph, const size_t &complexsize, double &m, double &d, double &g, const ColorCounts &counts, int device = 0,
          bool quiet = false);
    int ploidyEstimation_multithread_ptr(const std::string &outpre, const std::vector<std::pair<int, int>> &cutoff, const size_t &thr);

private:
    // the steps of the constructors: the colour sets and the commit gate; the colour sets the calling phase asks about
    bool init_colors();
    void colours_to_device();
    ColoredUnitigSet &cg_;
};

}  // namespace pfh
