// pfh::CDBG::findSuperBubble_multithread_ptr and the coverage launch it may start for the next phase.
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <stdexcept>
#include <thread>
#include <unordered_map>

#include "pf_cdbg_impl.hpp"
#include "pf_parallel.hpp"

namespace pfh {

size_t CDBG::host_threads(size_t thr) const { return threads_ ? threads_ : std::max<size_t>(thr, 1); }
// host walkers of the long traversals: each keeps 4 bytes of state per unitig, at most ~4 GiB of it in total
unsigned CDBG::walk_threads(size_t thr) const {
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(host_threads(thr), (4ull << 30) / (4ull * std::max<uint32_t>(g_.n(), 1))));
}

// Threads of the parallel commit replay: the single-sample path only (the colour gates of CCDBG's accept commit write NON_SUPER
// on endpoints, outside the footprint model), PF_REPLAY=seq or one thread keep the sequential loop.
unsigned CDBG::replay_threads(size_t thr) const {
    if (col_ != nullptr) return 0;
    static const char *env = getenv("PF_REPLAY");
    if (env && !strcmp(env, "seq")) return 0;
    static const int env_t = [] { const char *e = getenv("PF_REPLAY_THREADS"); return e ? atoi(e) : -1; }();
    int t = replay_threads_ >= 0 ? replay_threads_ : env_t >= 0 ? env_t : (int)std::min<size_t>(host_threads(thr), 32);
    return t >= 2 ? (unsigned)t : 0;
}

// The commits run on the device, one thread per component (pf_cc.hip), on the single-sample path unless the caller asked for
// host threads (set_replay_threads >= 0) or PF_REPLAY says host (components on host threads) or seq (the sequential loop).
bool CDBG::commits_on_device() const {
    if ((col_ != nullptr && !colours_on_device_) || !third_tier_on_host_ || replay_threads_ >= 0) return false;
    static const bool off = [] { const char *e = getenv("PF_REPLAY"); return e && (!strcmp(e, "host") || !strcmp(e, "seq")); }();
    static const bool env_threads = getenv("PF_REPLAY_THREADS") != nullptr;
    return !off && !env_threads;
}

int CDBG::sync_state_to_host() {
    if (!state_host_stale_) return 0;
    const int st = pf_call_get_state(ctx_, flags_.data(), plus_.data(), minus_.data());
    if (st != PF_OK) return fail(st, std::string(tag_) + "::findSuperBubble(): " + pf_last_error(ctx_));
    state_host_stale_ = false;
    return 0;
}

void CDBG::set_record_stats(const ReplayStats &s) {
    times_.bfs_large = s.large; times_.bfs_large_seen = s.large_seen; times_.bfs_max_seen = s.max_seen;
    times_.bfs_large_used = s.large_used; times_.bfs_large_used_max = s.large_used_max;
}

// One long traversal on a walker of the pool, with PF_TRACE_BFS's line (the resident path also says when the walk started).
void CDBG::walk_long(const FindTrace &tr, bool say_start, uint32_t entrance, pf_bfs_record &r, std::vector<uint32_t> &out) {
    const auto tw = clk::now();
    walkers_.walk(succ_.data(), pred_.data(), g_.n(), entrance, r, out);
    if (!tr.bfs) return;
    if (say_start)
        fprintf(stderr, "[bfs] host walk from %u: %u vertices, outcome %d, %.3f ms (started %.3f ms into findSuperBubble)\n", r.entrance, r.n_seen, (int)r.outcome, since(tw) * 1e3, (std::chrono::duration<double>(tw - tr.t_all).count()) * 1e3);
    else
        fprintf(stderr, "[bfs] host walk from %u: %u vertices, outcome %d, %.2f ms\n", r.entrance, r.n_seen, (int)r.outcome, since(tw) * 1e3);
}

// K-BFS leaves the traversals it gives up in deferred_ (record indices) and deferred_ent_ (their entrances), which keep their size
// from pass to pass: `call` runs one of its entry points, and runs again with longer lists while it reports more give-ups
// (n_deferred) than they hold.
template <class Call>
int CDBG::with_deferred(uint64_t &n_deferred, Call call) {
    if (deferred_.size() < 4096) deferred_.resize(4096);
    if (deferred_ent_.size() < deferred_.size()) deferred_ent_.resize(deferred_.size());
    for (;;) {
        const int st = call();
        if (st != PF_ERR_OVERFLOW || n_deferred <= deferred_.size()) return st;
        deferred_.resize(n_deferred + n_deferred / 4);
        deferred_ent_.resize(deferred_.size());
    }
}

// The sequential commit replay: `n` records in the reference's visiting order behind its `partner == NULL` gate (src/CDBG.cpp:206,
// 211); list_of(r) = the record's vertex list.
template <class ListOf>
void CDBG::replay_sequential(const pf_bfs_record *rec, uint64_t n, ListOf list_of, ReplayStats &stats) {
    for (uint64_t i = 0; i < n; ++i) {
        prefetch_commit_state(i, n, [&](uint64_t x) -> const pf_bfs_record & { return rec[x]; }, list_of, flags_.data(), 1, plus_.data(), minus_.data());
        const pf_bfs_record &r = rec[i];
        const bool open = st_.gate_open(r.entrance);
        stats.note(r, open);
        if (open) replay(r, list_of(r));
    }
}

// ---- findSuperBubble with the commits on the device --------------------------------------------------------------------------
// The long traversals are walked on host cores, side by side -- and from the moment the device gives each of them up: the wave
// tier reports its give-ups into pinned host memory as they happen (pf_bfs_live_deferred), the walkers started here poll it while
// pf_bfs_candidates_resident is still running.  The longest walk bounds this phase (136 k vertices = 2.7 ms at 5 M unitigs); it
// no longer waits for the device to finish with the other candidates first.  A walk is a function of its entrance alone, so the
// results are keyed by candidate index: whatever the live list missed (more give-ups than it holds, a repeated call after a pool
// overflow) is walked afterwards.  Every way out of the caller: the walkers learn that the list has ended, and are waited for.
struct CDBG::EarlyWalks {
    static constexpr uint64_t kCap = 4096;   // entries of the live list
    struct Walked {
        pf_bfs_record rec;
        std::vector<uint32_t> list;
        uint32_t cand = 0;   // candidate index + 1; 0 = slot unused
    };
    CDBG &g;
    const FindTrace &tr;
    volatile uint64_t *live = nullptr;
    std::vector<Walked> slots;
    std::atomic<uint64_t> next_slot{0};
    std::atomic<int64_t> final_n{-1};   // how many entries the live list ends with; -1 = the device is still at it
    std::string err;
    std::thread th;
    EarlyWalks(CDBG &g_, const FindTrace &tr_, unsigned threads) : g(g_), tr(tr_) {
        if (pf_bfs_live_deferred(g.ctx_, kCap, &live) != PF_OK) live = nullptr;
        if (!live) return;
        slots.resize(kCap);
        th = std::thread([this, threads] {
            try { parallel_chunks(threads, 1, threads, [this](size_t, size_t, size_t) { poll(); }); } catch (const std::exception &e) { err = e.what(); }
        });
    }
    ~EarlyWalks() { if (final_n.load() < 0) final_n.store(0); join(); }
    void list_ends_at(int64_t n) { final_n.store(n, std::memory_order_release); }
    void join() { if (th.joinable()) th.join(); }
    // one walker: the next entry of the live list, as soon as the device has written it, until the list ends
    void poll() {
        for (;;) {
            const uint64_t k = next_slot.fetch_add(1);
            if (k >= kCap) return;
            uint64_t e = 0;
            for (;;) {   // entry k, or the end of the list
                e = __atomic_load_n(const_cast<const uint64_t *>(&live[k]), __ATOMIC_ACQUIRE);
                if (e) break;
                const int64_t fn = final_n.load(std::memory_order_acquire);
                if (fn >= 0 && (int64_t)k >= fn) return;
                __builtin_ia32_pause();
            }
            Walked &wk = slots[(size_t)k];
            g.walk_long(tr, true, (uint32_t)(e >> 32), wk.rec, wk.list);
            wk.cand = (uint32_t)e;   // (index + 1)
        }
    }
};

// what the steps of find_superbubbles_device hand to each other
struct CDBG::DeviceFind {
    uint64_t n_rec = 0, n_deferred = 0, n_big = 0, big_entries = 0;
    // the long traversals: in deferred_'s order first, then (walked_into_candidate_order) in candidate order, the lists in xpool
    std::vector<pf_bfs_record> walked;
    std::vector<std::vector<uint32_t>> lists;
    std::vector<uint32_t> xpool;
    std::vector<uint32_t> p_sides;   // every side the host's commits wrote
};

// K-BFS over all candidates, records left in HBM; the early walkers learn where the live list ends
int CDBG::traverse_resident(EarlyWalks &early, DeviceFind &df, const FindTrace &tr) {
    uint64_t pool_used = 0;
    const int st = with_deferred(df.n_deferred, [&] {
        return pf_bfs_candidates_resident(ctx_, 0, g_.n(), &df.n_rec, &pool_used, deferred_.data(), deferred_ent_.data(), deferred_.size(), &df.n_deferred);
    });
    // (the live list holds notices: of every traversal that reached 48 vertices, whether the device gave it up afterwards or not)
    uint64_t n_live = 0;
    if (st == PF_OK && early.live) (void)pf_bfs_live_count(ctx_, &n_live);
    early.list_ends_at(st == PF_OK ? (int64_t)std::min<uint64_t>(n_live, EarlyWalks::kCap) : 0);
    if (tr.find) fprintf(stderr, "[find]   %llu notices in the live list, %llu traversals given up\n", (unsigned long long)n_live, (unsigned long long)df.n_deferred);
    return st;
}

// pair the early walks with the device's list by candidate index; walk what is left
void CDBG::walk_remaining(EarlyWalks &early, DeviceFind &df, const FindTrace &tr, unsigned threads) {
    early.join();
    if (!early.err.empty()) throw std::runtime_error(early.err);
    std::unordered_map<uint32_t, size_t> by_cand;
    for (size_t k = 0; k < early.slots.size(); ++k)
        if (early.slots[k].cand) by_cand.emplace(early.slots[k].cand - 1, k);
    std::vector<size_t> todo;
    for (size_t d = 0; d < (size_t)df.n_deferred; ++d) {
        auto it = by_cand.find(deferred_[d]);
        if (it != by_cand.end() && early.slots[it->second].rec.entrance == deferred_ent_[d]) {
            df.walked[d] = early.slots[it->second].rec;
            df.lists[d].swap(early.slots[it->second].list);
            by_cand.erase(it);
        } else {
            todo.push_back(d);
        }
    }
    if (!todo.empty())
        parallel_chunks(todo.size(), 1, threads, [&](size_t x, size_t, size_t) { walk_long(tr, true, deferred_ent_[todo[x]], df.walked[todo[x]], df.lists[todo[x]]); });
}

// in candidate order (the device hands the deferred candidates over in the order their wavefronts gave up)
void CDBG::walked_into_candidate_order(DeviceFind &df) {
    const size_t n = (size_t)df.n_deferred;
    std::vector<size_t> by_index(n);
    for (size_t d = 0; d < n; ++d) by_index[d] = d;
    std::sort(by_index.begin(), by_index.end(), [&](size_t a, size_t b) { return deferred_[a] < deferred_[b]; });
    std::vector<pf_bfs_record> w2(n);
    std::vector<uint32_t> d2(n);
    for (size_t i = 0; i < n; ++i) {
        const size_t d = by_index[i];
        w2[i] = df.walked[d];
        w2[i].list_off = df.xpool.size();
        w2[i].pad_ = 0;
        df.xpool.insert(df.xpool.end(), df.lists[d].begin(), df.lists[d].end());
        d2[i] = deferred_[d];
    }
    df.walked.swap(w2);
    std::copy(d2.begin(), d2.end(), deferred_.begin());
}

// what is left for this side: the records of the large components and of the components of the walked traversals, merged
// in record order
int CDBG::commit_large_on_host(DeviceFind &df, const FindTrace &tr, unsigned threads) {
    const uint32_t N = g_.n();
    const size_t n_big = (size_t)df.n_big, n_walked = (size_t)df.n_deferred;
    std::vector<uint32_t> big_idx(n_big);
    std::vector<pf_bfs_record> big_rec(n_big);
    std::vector<uint32_t> big_pool((size_t)df.big_entries + 1);
    const int st = pf_replay_big_fetch(ctx_, big_idx.data(), big_rec.data(), big_pool.data());
    if (st != PF_OK) return st;
    tr.step("large components fetched");
    if (big_f2_.size() != 2 * (size_t)N) big_f2_.assign(2 * (size_t)N, 0);
    // (plus_ / minus_ / big_f2_ are all-zero here: every pass undoes what it touched, see patch_device_state; a stale host copy is
    // re-zeroed)
    if (!state_host_stale_)
        parallel_chunks(N, 1u << 19, threads, [&](size_t, size_t b, size_t e) {
            memset(plus_.data() + b, 0, (e - b) * 4);
            memset(minus_.data() + b, 0, (e - b) * 4);
        });
    // (every side written is noted: exactly those go to the device afterwards)
    const FlagsPerSideLogged acc{FlagsPerSide{big_f2_.data(), plus_.data(), minus_.data()}, &df.p_sides};
    Commits<FlagsPerSideLogged> cm{acc, complex_size_, NoColours{}};
    Commits<FlagsPerSideLogged, ColourGate> cmc{acc, complex_size_, col_ ? st_.colour_gate() : ColourGate{}};
    ReplayStats stats;
    auto commit = [&](const pf_bfs_record &r, const uint32_t *list) {   // true: the record took effect
        const bool effective = record_effective(r) && cm.gate_open(r.entrance);
        stats.note(r, effective);
        if (effective) { if (col_) cmc.replay(r, list); else cm.replay(r, list); }
        return effective;
    };
    // (for the trace, [0] the large components' records and [1] the walked ones: time, records that took effect, their list entries)
    double t[2] = {0, 0};
    uint64_t eff[2] = {0, 0}, ent[2] = {0, 0};
    size_t a = 0, b = 0;   // a over big_idx, b over the walked records (ascending candidate index both)
    while (a < n_big || b < n_walked) {
        const bool w = a >= n_big || (b < n_walked && deferred_[b] < big_idx[a]);
        const auto tc = tr.find ? clk::now() : clk::time_point();
        const pf_bfs_record &r = w ? df.walked[b++] : big_rec[a++];
        if (commit(r, (w ? df.xpool.data() : big_pool.data()) + r.list_off)) { ent[w] += r.n_list; ++eff[w]; }
        if (tr.find) t[w] += since(tc);
    }
    set_record_stats(stats);
    if (tr.find)
        fprintf(stderr, "[find]   replayed here: %zu walked records (%llu take effect, %llu list entries) %.3f ms, %llu records of large components (%llu, %llu) %.3f ms\n",
                n_walked, (unsigned long long)eff[1], (unsigned long long)ent[1], t[1] * 1e3, (unsigned long long)df.n_big, (unsigned long long)eff[0], (unsigned long long)ent[0], t[0] * 1e3);
    tr.step("large components replayed");
    return PF_OK;
}

// The sides the host's commits wrote go into the device's state; beside that the host arrays go back to all-zero for the next
// pass (the device's patch reads the gathered copies only).
int CDBG::patch_device_state(const std::vector<uint32_t> &sides, const FindTrace &tr, unsigned threads) {
    std::vector<uint32_t> links(sides.size());
    std::vector<uint8_t> bytes(sides.size());
    parallel_chunks(sides.size(), 1u << 14, threads, [&](size_t, size_t b, size_t e) {
        for (size_t i = b; i < e; ++i) {
            const uint32_t s = sides[i];
            links[i] = (s & 1) ? minus_[s >> 1] : plus_[s >> 1];
            bytes[i] = big_f2_[s];
        }
    });
    tr.step("patch gathered");
    std::thread undo([&] {
        parallel_chunks(sides.size(), 1u << 14, threads, [&](size_t, size_t b, size_t e) {
            for (size_t i = b; i < e; ++i) {   // (a side logged twice may be zeroed from two threads: relaxed atomic stores of the same value)
                const uint32_t s = sides[i];
                __atomic_store_n(&((s & 1) ? minus_ : plus_)[s >> 1], 0u, __ATOMIC_RELAXED);
                __atomic_store_n(&big_f2_[s], (uint8_t)0, __ATOMIC_RELAXED);
            }
        });
    });
    const int st = pf_replay_finish(ctx_, sides.data(), links.data(), bytes.data(), sides.size());
    undo.join();
    return st;
}

// findSuperBubble with nothing but the long traversals on the host: K-BFS leaves its records in HBM, K-CC finds the components,
// pf_replay_device commits every small component with one thread; the few large ones (and those of the traversals walked here)
// are committed on this side and their sides patched into the device state.
int CDBG::find_superbubbles_device(const std::string &outpre, const size_t &thr) {
    const FindTrace tr;
    auto failed = [&](int st) { return fail(st, std::string("CDBG::findSuperBubble(): ") + pf_last_error(ctx_)); };
    out_bytes_ = 0;
    state_on_device_ = false;
    cov_ready_ = false;
    for (auto &hl : huge_lists_) hl.clear();
    const unsigned wt = walk_threads(thr), few = (unsigned)std::min<size_t>(host_threads(thr), 8);
    DeviceFind df;
    EarlyWalks early(*this, tr, wt);
    int st = traverse_resident(early, df, tr);
    if (st != PF_OK) return failed(st);
    tr.step("traversed on the device");
    df.walked.resize((size_t)df.n_deferred);
    df.lists.resize((size_t)df.n_deferred);
    std::string walk_err;
    std::thread walk([&] { try { walk_remaining(early, df, tr, wt); } catch (const std::exception &e) { walk_err = e.what(); } });
    // K-CC over the records that are on the device, beside the walkers
    st = pf_side_components(ctx_, 1, nullptr, df.n_rec, nullptr, 0, nullptr, 0, nullptr, 0);
    tr.step("  components of the device's records");
    // ... and the coverage kernel PloidyEstimation starts with (it depends on nothing this phase computes)
    if (st == PF_OK && overlap_output_) cov_ready_ = launch_coverage() == PF_OK;
    tr.step("  coverage launched");
    walk.join();
    if (!walk_err.empty()) return fail(PF_ERR_HIP, "CDBG::findSuperBubble(): walk of a long traversal: " + walk_err);
    if (st != PF_OK) return failed(st);
    tr.step("long traversals walked");
    walked_into_candidate_order(df);
    tr.step("  walked records in candidate order");
    if (!df.walked.empty()) st = pf_side_components(ctx_, 0, nullptr, df.n_rec, nullptr, 0, df.walked.data(), df.walked.size(), df.xpool.data(), df.xpool.size());
    tr.step("  their components");
    // (PF_REPLAY_SMALL_LIMIT: tests push more components -- all of them with 0 -- through the host half and its patch)
    static const uint32_t small_limit = [] { const char *e = getenv("PF_REPLAY_SMALL_LIMIT"); return e ? (uint32_t)atoi(e) : 256u; }();
    if (st == PF_OK) st = pf_replay_device(ctx_, (uint32_t)std::min<size_t>(complex_size_, 0xFFFFFFFFu), small_limit, &df.n_big, &df.big_entries);
    if (st != PF_OK) return failed(st);
    tr.step("components + commits on the device");
    st = commit_large_on_host(df, tr, few);
    if (st != PF_OK) return failed(st);
    st = patch_device_state(df.p_sides, tr, few);
    if (st != PF_OK) return failed(st);
    if (tr.find) fprintf(stderr, "[find] %zu sides patched on the device %.2f ms\n", df.p_sides.size(), since(tr.t_all) * 1e3);
    state_host_stale_ = true;
    state_on_device_ = true;
    tr.step("large components committed here");
    times_.bfs_device_s = since(tr.t_all);
    times_.candidates = df.n_rec;
    times_.bfs_deferred = df.n_deferred;
    times_.host_commit_records = df.n_big + df.n_deferred;
    times_.host_walk_vertices = 0;
    for (const auto &w : df.walked) times_.host_walk_vertices += w.n_seen;
    times_.replay_s = 0;
    return finish_find(outpre, tr, write_sb_, true);
}

// ---- findSuperBubble (reference src/CDBG.cpp:178-252) -------------------------------------
// Every candidate entrance is traversed on the device, one wavefront each.  The unitig range is cut into slices:
// a helper thread (the only one issuing device calls here, traverse_slices) runs K-BFS slice by slice and, after the last one,
// the coverage kernel PloidyEstimation starts with -- while the calling thread replays the records of the finished slices in
// the reference's visiting order, with its `partner == NULL` gate (src/CDBG.cpp:206, 211): records come in
// ascending oriented-vertex order = unitig order, '+' before '-'.
struct CDBG::SlicedFind {
    static constexpr int kMaxSlices = 4;
    int n_slices = 1;
    unsigned rt = 0, walk_threads = 1;   // threads of the parallel replay (0 = sequential) and of the host walkers
    uint32_t u0[kMaxSlices + 1];
    uint64_t rec0[kMaxSlices + 1], pool0[kMaxSlices + 1], n_rec[kMaxSlices], used[kMaxSlices];
    uint32_t class_off[kMaxSlices][kReplayClasses + 1];
    std::unique_ptr<PinnedBuf<uint32_t>> own_pool[kMaxSlices];   // a slice whose pool guess was too small gets a buffer of its own
    const uint32_t *pool[kMaxSlices];
    // from the device thread to the replay: slices [0, done) are complete, or the device thread has failed
    std::mutex mu; std::condition_variable cv;
    int done = 0, dev_st = PF_OK;
    std::string dev_err;
    double bfs_s = 0;
    uint64_t n_deferred_total = 0;
};

// K-BFS over slice i: the device's tiers, the long traversals on host cores beside K-CC and the copy of the records, and (parallel
// replay) the slice's commit order
int CDBG::traverse_slice(SlicedFind &sf, int i, const FindTrace &tr) {
    const auto tb = clk::now();
    pf_bfs_record *rec = bx_.bfs_rec.p + sf.rec0[i];
    const uint64_t rec_cap = sf.rec0[i + 1] - sf.rec0[i];
    uint32_t *pl = bx_.bfs_pool.p + sf.pool0[i];
    uint64_t cap = sf.pool0[i + 1] - sf.pool0[i];
    uint64_t n_deferred = 0;
    int st1;
    for (;;) {
        if (third_tier_on_host_)
            // the records travel to the host while the long traversals are walked (pf_bfs_candidates_end below)
            st1 = with_deferred(n_deferred, [&] {
                return pf_bfs_candidates_begin(ctx_, sf.u0[i], sf.u0[i + 1], rec, rec_cap, pl, cap, &sf.n_rec[i], &sf.used[i], deferred_.data(), deferred_ent_.data(), deferred_.size(), &n_deferred);
            });
        else
            st1 = pf_bfs_candidates(ctx_, sf.u0[i], sf.u0[i + 1], rec, rec_cap, pl, cap, &sf.n_rec[i], &sf.used[i]);
        if (st1 != PF_ERR_OVERFLOW || sf.used[i] <= cap) break;
        sf.own_pool[i] = std::make_unique<PinnedBuf<uint32_t>>();
        sf.own_pool[i]->ensure(ctx_, sf.used[i] + sf.used[i] / 8);
        pl = sf.own_pool[i]->p;
        cap = sf.own_pool[i]->cap;
    }
    sf.pool[i] = pl;
    sf.n_deferred_total += n_deferred;
    if (tr.bfs) fprintf(stderr, "[bfs] device tiers of slice %d: %.2f ms, %llu candidates left for the third tier\n", i, since(tb) * 1e3, (unsigned long long)n_deferred);
    std::vector<pf_bfs_record> walked((size_t)n_deferred);
    std::string walk_err;
    std::thread walk;
    if (st1 == PF_OK && n_deferred) {
        // third tier: one host thread per giant traversal, side by side; lists go to huge_lists_
        huge_lists_[i].assign((size_t)n_deferred, std::vector<uint32_t>());
        walk = std::thread([&] {
            try {
                parallel_chunks((size_t)n_deferred, 1, sf.walk_threads, [&](size_t d, size_t, size_t) {
                    walk_long(tr, false, deferred_ent_[d], walked[d], huge_lists_[i][d]);
                    walked[d].list_off = d; walked[d].pad_ = 1;
                });
            } catch (const std::exception &e) { walk_err = e.what(); }
        });
    }
    // K-CC for the records that are on the device, beside the walkers and the copy
    if (st1 == PF_OK && sf.rt) st1 = pf_side_components(ctx_, i == 0, nullptr, sf.n_rec[i], nullptr, 0, nullptr, 0, nullptr, 0);
    if (walk.joinable()) walk.join();
    if (!walk_err.empty()) throw std::runtime_error("walk of a long traversal: " + walk_err);
    if (third_tier_on_host_) {
        const int ste = pf_bfs_candidates_end(ctx_);
        if (st1 == PF_OK) st1 = ste;
    }
    if (st1 == PF_OK)
        for (uint64_t d = 0; d < n_deferred; ++d) rec[deferred_[d]] = walked[(size_t)d];
    const auto t_cc = clk::now();
    if (tr.find) fprintf(stderr, "[find]   slice %d traversed (%llu records, %llu walked on host cores) %.2f ms (+%.2f)\n", i, (unsigned long long)sf.n_rec[i],
                         (unsigned long long)n_deferred, since(tr.t_all) * 1e3, since(tb) * 1e3);
    if (st1 == PF_OK && sf.rt) {
        // K-CC: the slice's records join the components (they are still on the device; the traversals walked on the host
        // add their footprints from here), then the slice's commit order by component class
        std::vector<pf_bfs_record> xrec;
        std::vector<uint32_t> xpool;
        for (uint64_t d = 0; d < n_deferred; ++d) {
            pf_bfs_record r = rec[deferred_[d]];
            const std::vector<uint32_t> &l = huge_lists_[i][(size_t)d];
            r.list_off = xpool.size();
            r.pad_ = 0;
            xpool.insert(xpool.end(), l.begin(), l.begin() + r.n_list);
            xrec.push_back(r);
        }
        if (!xrec.empty()) st1 = pf_side_components(ctx_, 0, nullptr, sf.n_rec[i], nullptr, 0, xrec.data(), xrec.size(), xpool.data(), xpool.size());
        if (st1 == PF_OK) st1 = pf_replay_order(ctx_, kReplayClasses, bx_.bfs_order.p + sf.rec0[i], sf.class_off[i], nullptr);
        if (tr.find) fprintf(stderr, "[find]   slice %d components + order %.2f ms (+%.2f)\n", i, since(tr.t_all) * 1e3, since(t_cc) * 1e3);
    }
    sf.bfs_s += since(tb);
    return st1;
}

// the device thread of the sliced pass: slice after slice, each handed to the replay when it is complete
void CDBG::traverse_slices(SlicedFind &sf, const FindTrace &tr) {
    try {
        for (int i = 0; i < sf.n_slices; ++i) {
            const int st1 = traverse_slice(sf, i, tr);
            {
                std::lock_guard<std::mutex> lk(sf.mu);
                if (st1 != PF_OK) { sf.dev_st = st1; sf.dev_err = pf_last_error(ctx_); }
                sf.done = i + 1;
            }
            sf.cv.notify_all();
            if (st1 != PF_OK) return;
        }
        if (overlap_output_) cov_ready_ = launch_coverage() == PF_OK;
    } catch (const std::exception &e) {   // (bad_alloc of a list or a buffer: reported like a device error, not std::terminate)
        (void)pf_bfs_candidates_end(ctx_);   // (a copy of records may still be in flight)
        {
            std::lock_guard<std::mutex> lk(sf.mu);
            sf.dev_st = PF_ERR_HIP;
            sf.dev_err = std::string("host layer: ") + e.what();
        }
        sf.cv.notify_all();
    }
}

int CDBG::findSuperBubble_multithread_ptr(const std::string &outpre, const size_t &thr) {
    if (status_) return status_;
    join_prealloc();
    if (join_pending_write()) return status_;
    if (!quiet_) printf("%s::findSuperBubble(): Finding superbubbles\n", tag_);
    if (write_files_ && ensure_dir()) return status_;
    const uint32_t N = g_.n();
    if (!quiet_) printf("%s::findSuperBubble(): There are %u unitigs \n", tag_, N);
    if (commits_on_device()) return find_superbubbles_device(outpre, thr);
    state_host_stale_ = false;
    const FindTrace tr;
    out_bytes_ = 0;
    state_on_device_ = false;
    SlicedFind sf;
    const unsigned rt = sf.rt = replay_threads(thr);
    sf.walk_threads = walk_threads(thr);
    const unsigned zt = std::max<unsigned>(rt, (unsigned)std::min<size_t>(host_threads(thr), 8));
    parallel_chunks(N, 1u << 19, zt, [&](size_t, size_t b, size_t e) {
        memset(flags_.data() + b, 0, e - b);
        memset(plus_.data() + b, 0, (e - b) * 4);
        memset(minus_.data() + b, 0, (e - b) * 4);
    });
    if (rt) par_.begin(N, plus_.data(), minus_.data(), complex_size_, rt);
    // The unitig range is cut into slices so that the replay of slice i overlaps the traversal of slice i + 1.  With the long
    // traversals on host cores a slice's own are walked in a few milliseconds, side by side; only with the device's third tier
    // (one wavefront per giant traversal, run slice after slice) is the first pass over a graph kept in one piece.
    // (with the commits spread over host threads a slice's replay takes a millisecond: slicing only pays for the sequential replay)
    const int kSlices = sf.n_slices = rt ? 1 : (third_tier_on_host_ || (find_passes_ > 0 && times_.bfs_large == 0)) ? SlicedFind::kMaxSlices : 1;
    ++find_passes_;
    sf.rec0[0] = sf.pool0[0] = 0;
    for (int i = 0; i <= kSlices; ++i) sf.u0[i] = (uint32_t)((uint64_t)N * i / kSlices);
    for (int i = 0; i < kSlices; ++i) {
        uint64_t n_cand = 0;
        int st0 = pf_count_candidates(ctx_, sf.u0[i], sf.u0[i + 1], &n_cand);
        if (st0 != PF_OK) return fail(st0, pf_last_error(ctx_));
        sf.rec0[i + 1] = sf.rec0[i] + std::max<uint64_t>(n_cand, 1);
        sf.pool0[i + 1] = sf.pool0[i] + n_cand * 6 + (1u << 20);   // the pool guess leaves room for the per-wave chunk slack
        sf.n_rec[i] = sf.used[i] = 0;
    }
    tr.step("candidates counted");
    bx_.bfs_rec.ensure(ctx_, sf.rec0[kSlices]);   // pinned, reused from pass to pass
    bx_.bfs_pool.ensure(ctx_, sf.pool0[kSlices]);
    if (rt) bx_.bfs_order.ensure(ctx_, sf.rec0[kSlices]);
    tr.step("pinned record buffers");
    cov_ready_ = false;
    static_assert(SlicedFind::kMaxSlices <= 4, "huge_lists_ holds four slices");
    for (auto &hl : huge_lists_) hl.clear();
    std::thread device([&] { traverse_slices(sf, tr); });
    ReplayStats stats;
    set_record_stats(stats);   // (kSlices above looked at the previous pass)
    times_.bfs_deferred = 0;
    uint64_t n_rec_total = 0;
    double replay_s = 0;
    int st = PF_OK;
    for (int sl = 0; sl < kSlices; ++sl) {
        {
            std::unique_lock<std::mutex> lk(sf.mu);
            sf.cv.wait(lk, [&] { return sf.done > sl || sf.dev_st != PF_OK; });
            if (sf.done <= sl || (sf.dev_st != PF_OK && sf.done == sl + 1)) { st = sf.dev_st; break; }
        }
        const auto t0 = clk::now();
        const pf_bfs_record *srec = bx_.bfs_rec.p + sf.rec0[sl];
        const uint32_t *pool = sf.pool[sl];
        n_rec_total += sf.n_rec[sl];
        auto list_of = [&](const pf_bfs_record &r) { return r.pad_ ? huge_lists_[sl][r.list_off].data() : pool + r.list_off; };
        if (rt) {
            par_.run(srec, list_of, bx_.bfs_order.p + sf.rec0[sl], sf.class_off[sl], kReplayClasses, rt, stats);
            if (tr.find) fprintf(stderr, "[find]   slice %d replayed on %u threads %.2f ms (+%.2f)\n", sl, rt, since(tr.t_all) * 1e3, since(t0) * 1e3);
        } else replay_sequential(srec, sf.n_rec[sl], list_of, stats);
        replay_s += since(t0);
    }
    if (rt && st == PF_OK) {
        const auto t0 = clk::now();
        par_.finish(flags_.data(), rt);
        replay_s += since(t0);
    }
    tr.step("replay done");
    device.join();
    tr.step("device thread joined");
    if (st != PF_OK || sf.dev_st != PF_OK) return fail(sf.dev_st != PF_OK ? sf.dev_st : st, std::string("CDBG::findSuperBubble(): ") + sf.dev_err);
    set_record_stats(stats);
    times_.bfs_device_s = sf.bfs_s;
    times_.candidates = n_rec_total;
    times_.bfs_deferred = sf.n_deferred_total;
    times_.replay_s = replay_s;
    return finish_find(outpre, tr, write_sb_, true);
}

// second half of findSuperBubble (reference src/CDBG.cpp:222-252): the rows of <outpre>_super_bubble.txt from the final state
int CDBG::finish_find(const std::string &outpre, const FindTrace &tr, bool write_file, bool timing_lines) {
    if (timing_lines && !quiet_) {
        // (the reference words these two lines differently in its threaded function, src/CDBG.cpp:1783-1786)
        printf(mt_format_ ? "%s::findSuperBubble(): Finding superbubbles Cpu time : %gs\n" : "%s::findSuperBubble():  Cpu time : %gs\n", tag_,
               (double)(clock() - tr.cpu0) / CLOCKS_PER_SEC);
        printf(mt_format_ ? "%s::findSuperBubble(): Finding superbubbles Real time : %gs\n" : "%s::findSuperBubble():  Real time : %gs\n", tag_,
               since(tr.t_all));
    }
    auto t0 = clk::now();
    // The state goes to the device once -- PloidyEstimation's scan reads it there as well -- and the rows of super_bubble.txt
    // (one per open endpoint side in unitig order, numbered by a prefix count) are formatted there; the text comes back and is
    // written by a helper thread, behind the caller's back when overlap_output is on.
    int st = state_on_device_ ? PF_OK : pf_call_set_state(ctx_, flags_.data(), plus_.data(), minus_.data());
    uint64_t nb = 0, len = 0;
    if (st == PF_OK) st = pf_superbubble_rows(ctx_, col_ != nullptr ? 1 : 0, &nb, &len);
    if (st != PF_OK) return fail(st, std::string(tag_) + "::findSuperBubble(): " + pf_last_error(ctx_));
    state_on_device_ = true;
    tr.step("super_bubble rows on the device");
    static const char kHeader[] = "BubbleId\tEntrance\tStrand\tExit\tisSimple\tisComplex\n";
    n_super_bubble_ = nb;
    times_.bubbles_out = nb;
    out_bytes_ += len + (sizeof(kHeader) - 1);
    if (write_file && write_files_) {
        join_pending_write();
        sb_text_.ensure(ctx_, std::max<uint64_t>(len, 1));
        const unsigned T = (unsigned)host_threads(1);
        auto job = [this, name = outpre + "_super_bubble.txt", len, T, trace_find = tr.find]() -> int {
            const auto tj = clk::now();
            if (pf_superbubble_fetch(ctx_, sb_text_.p, len) != PF_OK) return 1;
            const double t_fetch = since(tj);
            MappedOut &mo = out_maps_[PF_CALL_STREAMS];   // (the slot after the ten streams of PloidyEstimation)
            if (mo.open_for(outdir_ + "/" + name)) return 1;
            const uint64_t hl = sizeof(kHeader) - 1;
            int rc = mo.write(0, kHeader, hl, 1);
            rc |= mo.write(hl, sb_text_.p, len, T);
            rc |= mo.finish(hl + len);
            if (trace_find) fprintf(stderr, "[find]   super_bubble.txt: fetched after %.2f ms, in the file after %.2f ms (%.1f MB)\n", t_fetch * 1e3, since(tj) * 1e3, len / 1e6);
            return rc;
        };
        if (overlap_output_) {
            // written behind the caller's back while PloidyEstimation starts; joined there (or by the next use of the file)
            pending_write_ = std::thread([this, job] { pending_rc_ = job(); });
        } else if (job()) {
            return fail(PF_ERR_ARG, "CDBG:: Open " + outpre + "_super_bubble.txt file error");
        }
    }
    times_.bubble_write_s = since(t0);
    times_.find_total_s = since(tr.t_all);
    tr.step("super_bubble rows done");
    if (!quiet_) printf("%s::findSuperBubble(): %llu  SuperBubbles Found\n", tag_, (unsigned long long)nb);
    return 0;
}

// ---- one graph over several GPUs: a rank traverses the candidate entrances of its unitig range only ----
// K-BFS (LDS tier on the device, the long traversals on host cores) for the entrances on unitigs [u0, u1); the records and their
// vertex lists are left self-contained in shard_rec_ / shard_pool_ (list_off relative to shard_pool_) for the exchange.
int CDBG::find_shard(uint32_t u0, uint32_t u1) {
    if (status_) return status_;
    join_prealloc();
    const uint32_t N = g_.n();
    if (u0 > u1 || u1 > N) return fail(PF_ERR_ARG, "CDBG::find_shard(): range outside the graph");
    const auto tb = clk::now();
    uint64_t n_cand = 0;
    int st = pf_count_candidates(ctx_, u0, u1, &n_cand);
    if (st != PF_OK) return fail(st, pf_last_error(ctx_));
    bx_.bfs_rec.ensure(ctx_, std::max<uint64_t>(n_cand, 1));
    bx_.bfs_pool.ensure(ctx_, n_cand * 6 + (1u << 20));
    uint64_t n_rec = 0, used = 0, n_deferred = 0;
    for (;;) {
        st = with_deferred(n_deferred, [&] {
            return pf_bfs_candidates_split(ctx_, u0, u1, bx_.bfs_rec.p, bx_.bfs_rec.cap, bx_.bfs_pool.p, bx_.bfs_pool.cap, &n_rec, &used, deferred_.data(), deferred_.size(),
                                           &n_deferred);
        });
        if (st != PF_ERR_OVERFLOW || used <= bx_.bfs_pool.cap) break;
        bx_.bfs_pool.ensure(ctx_, used + used / 8);
    }
    if (st != PF_OK) return fail(st, std::string("CDBG::findSuperBubble(): ") + pf_last_error(ctx_));
    shard_rec_.assign(bx_.bfs_rec.p, bx_.bfs_rec.p + n_rec);
    shard_pool_.assign(bx_.bfs_pool.p, bx_.bfs_pool.p + used);
    if (n_deferred) {
        std::vector<std::vector<uint32_t>> lists((size_t)n_deferred);
        parallel_chunks((size_t)n_deferred, 1, walk_threads(1), [&](size_t d, size_t, size_t) {
            pf_bfs_record &r = shard_rec_[deferred_[d]];
            walkers_.walk(succ_.data(), pred_.data(), N, r.entrance, r, lists[d]);
        });
        for (size_t d = 0; d < (size_t)n_deferred; ++d) {
            pf_bfs_record &r = shard_rec_[deferred_[d]];
            r.list_off = shard_pool_.size();
            r.pad_ = 0;
            shard_pool_.insert(shard_pool_.end(), lists[d].begin(), lists[d].end());
        }
    }
    times_.bfs_device_s = since(tb);
    times_.bfs_deferred = n_deferred;
    return 0;
}

// The commit replay over the records of all shards, in shard order = entrance order (reference visiting order, src/CDBG.cpp:
// 206-214), then the rows of super_bubble.txt; every rank ends with the same state.
int CDBG::find_replay(const std::string &outpre, uint32_t n_shards, const pf_bfs_record *const *records, const uint64_t *n_records,
                      const uint32_t *const *pools, bool write_file, const uint64_t *pool_lens, const pf_bfs_record *const *dev_records,
                      const uint32_t *const *dev_pools) {
    if (status_) return status_;
    if (join_pending_write()) return status_;
    if (write_file && write_files_ && ensure_dir()) return status_;
    const FindTrace tr;
    out_bytes_ = 0;
    state_on_device_ = false;
    state_host_stale_ = false;
    std::fill(flags_.begin(), flags_.end(), 0);
    std::fill(plus_.begin(), plus_.end(), 0);
    std::fill(minus_.begin(), minus_.end(), 0);
    cov_ready_ = false;
    ReplayStats stats;
    set_record_stats(stats);
    const auto t0 = clk::now();
    uint64_t total = 0;
    uint32_t last = 0;
    // the parallel replay needs the lengths of the pools (the device refuses lists outside them)
    const unsigned rt = pool_lens ? replay_threads(1) : 0;
    if (rt) par_.begin(g_.n(), plus_.data(), minus_.data(), complex_size_, rt);
    std::vector<uint32_t> order;
    // shards given as device memory only (the all-gather's output): their host copies come down into the pinned exchange buffers
    std::vector<const pf_bfs_record *> h_rec(n_shards);
    std::vector<const uint32_t *> h_pool(n_shards);
    {
        uint64_t need_rec = 0, need_pool = 0;
        for (uint32_t sh = 0; sh < n_shards; ++sh) {
            h_rec[sh] = records ? records[sh] : nullptr;
            h_pool[sh] = pools ? pools[sh] : nullptr;
            if (!h_rec[sh] || !h_pool[sh]) {
                if (!pool_lens || !dev_records || !dev_pools || !dev_records[sh] || !dev_pools[sh])
                    return fail(PF_ERR_ARG, "CDBG::find_replay(): a shard has neither host nor device arrays");
                need_rec += n_records[sh];
                need_pool += pool_lens[sh];
            }
        }
        if (need_rec) {
            bx_.bfs_rec.ensure(ctx_, need_rec + 1);
            bx_.bfs_pool.ensure(ctx_, need_pool + 1);
            uint64_t ar = 0, ap = 0;
            for (uint32_t sh = 0; sh < n_shards; ++sh) {
                if (h_rec[sh] && h_pool[sh]) continue;
                int st = pf_fetch(ctx_, bx_.bfs_rec.p + ar, dev_records[sh], n_records[sh] * sizeof(pf_bfs_record));
                if (st == PF_OK) st = pf_fetch(ctx_, bx_.bfs_pool.p + ap, dev_pools[sh], pool_lens[sh] * 4);
                if (st != PF_OK) return fail(st, std::string("CDBG::find_replay(): ") + pf_last_error(ctx_));
                h_rec[sh] = bx_.bfs_rec.p + ar;
                h_pool[sh] = bx_.bfs_pool.p + ap;
                ar += n_records[sh];
                ap += pool_lens[sh];
            }
        }
    }
    for (uint32_t sh = 0; sh < n_shards; ++sh) {
        const pf_bfs_record *rec = h_rec[sh];
        const uint32_t *pool = h_pool[sh];
        const uint64_t n = n_records[sh];
        total += n;
        for (uint64_t i = 0; i < n; ++i) {   // (`last` starts at 0: the first record of all passes whatever its entrance)
            const pf_bfs_record &r = rec[i];
            if ((r.entrance >> 1) >= g_.n() || r.entrance < last) return fail(PF_ERR_ARG, "CDBG::find_replay(): records out of order");
            last = r.entrance;
        }
        auto list_of = [&](const pf_bfs_record &r) { return pool + r.list_off; };
        if (!rt) { replay_sequential(rec, n, list_of, stats); continue; }
        const bool on_dev = dev_records && dev_pools && dev_records[sh] && dev_pools[sh];
        int st = pf_side_components(ctx_, sh == 0, on_dev ? dev_records[sh] : rec, n, on_dev ? dev_pools[sh] : pool, pool_lens[sh], nullptr, 0, nullptr, 0);
        uint32_t class_off[kReplayClasses + 1];
        order.resize(std::max<uint64_t>(n, 1));
        if (st == PF_OK) st = pf_replay_order(ctx_, kReplayClasses, order.data(), class_off, nullptr);
        if (st != PF_OK) return fail(st, std::string("CDBG::find_replay(): ") + pf_last_error(ctx_));
        par_.run(rec, list_of, order.data(), class_off, kReplayClasses, rt, stats);
    }
    if (rt) par_.finish(flags_.data(), rt);
    stats.large_used = stats.large_used_max = 0;   // (this call has never reported the two: they stay at zero)
    set_record_stats(stats);
    times_.replay_s = since(t0);
    times_.candidates = total;
    return finish_find(outpre, tr, write_file, false);
}

// K-COV (colored: K-COV-C) for all unitigs into the pinned result buffers.  A missing k-mer is not an error here: the
// single-sample path raises it only for the unitigs it really uses, the colored path never (src/CCDBG.cpp:113-117).
int CDBG::launch_coverage() {
    if (resident_path()) {  // the results stay on the device, where the scan of the calling pipeline reads them
        const int st = pf_call_coverage(ctx_);
        if (st != PF_OK) cov_err_ = pf_last_error(ctx_);
        return st;
    }
    const uint32_t N = g_.n();
    // a database without canonical counting (single-sample only) is read per orientation: [0, N) the unitigs as stored,
    // [N, 2N) their reverse complements (readCov(UnitigMap), src/CDBG.cpp:94-117)
    const uint32_t C = col_ ? col_->n_colors : (both_strands_ ? 1 : 2);
    bx_.cov_sum.ensure(ctx_, (size_t)N * C);
    bx_.cov_min.ensure(ctx_, (size_t)N * C);
    bx_.cov_miss.ensure(ctx_, (size_t)N * C);
    if (col_) bx_.cov_max.ensure(ctx_, (size_t)N * C);
    int st;
    if (col_) st = pf_unitig_cov_colored(ctx_, 0, N, bx_.cov_sum.p, bx_.cov_min.p, bx_.cov_max.p, bx_.cov_miss.p);
    else if (both_strands_) st = pf_unitig_cov(ctx_, 0, N, bx_.cov_sum.p, bx_.cov_min.p, bx_.cov_miss.p);
    else {
        st = pf_unitig_cov_exact(ctx_, 0, N, 0, bx_.cov_sum.p, bx_.cov_min.p, bx_.cov_miss.p);
        if (st == PF_OK || st == PF_ERR_MISSING_KMER) st = pf_unitig_cov_exact(ctx_, 0, N, 1, bx_.cov_sum.p + N, bx_.cov_min.p + N, bx_.cov_miss.p + N);
    }
    if (st != PF_OK && st != PF_ERR_MISSING_KMER) { cov_err_ = pf_last_error(ctx_); return st; }
    return PF_OK;
}

}  // namespace pfh
