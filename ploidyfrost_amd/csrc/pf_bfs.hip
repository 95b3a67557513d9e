// K-BFS: superbubble traversal of every candidate entrance (CDBG::extractSuperBubble_ptr, src/CDBG.cpp:253-372), the device half
// of findSuperBubble.  The traversal itself is in pf_bfs.hpp / pf_bfs_huge.hpp; here are the tiers that run it and their driver:
//   thread tier     k_bfs_thread   one thread per candidate, 8-entry tables
//   wavefront tier  k_bfs          one wavefront per candidate the thread tier passed on, 128-entry tables in LDS
//   big tier        k_bfs_big      what outgrew those, linear tables of 4096 entries in global scratch
//   huge tier       k_bfs_huge     what outgrew those too, direct-indexed state sized by the graph
// The first two run in every call.  What they give up is either run on the last two or handed to the caller (BfsMode).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "pf_bfs.hpp"
#include "pf_bfs_huge.hpp"
#include "pf_ctx.hpp"

using namespace pf;

// ------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------

// K-BFS, LDS tier: 4 waves per block, each with its own LDS slice of CAP entries.
constexpr uint32_t BFS_LDS_CAP = 128;
constexpr uint32_t BFS_BIG_CAP = 1u << 12;  // linear-scan tables: beyond this the direct-indexed tier takes over

struct BfsOut {
    pf_bfs_record *rec;
    uint32_t *pool;
    uint64_t pool_cap;
    unsigned long long *pool_head;  // running total (may exceed pool_cap: tells the size needed)
    uint32_t *deferred;             // candidate indices for the big tier
    unsigned int *n_deferred;
    uint32_t *deferred2;            // ... and for the direct-indexed tier
    unsigned int *n_deferred2;
    // pf_bfs_live_deferred: the same hand-over, at once, in host memory the caller polls while the kernel runs: entry d =
    // entrance << 32 | (candidate index + 1)
    unsigned long long *live;
    uint32_t live_cap;
    unsigned int *n_live;   // entries of the live list (notices of traversals still running on the device included)
    uint32_t hint_at;       // a traversal is entered when it reaches this many vertices
};

// Per-wave bump allocation in the vertex pool: a wave reserves BFS_POOL_CHUNK entries with one
// atomic and hands them out locally, so the single pool head is touched once per ~50 candidates instead
// of once per candidate (one hot word saturates at ~90 atomics/us chip-wide).
constexpr uint32_t BFS_POOL_CHUNK = 256;
struct BfsAlloc {
    unsigned long long cur = 0, end = 0;
};

__device__ inline void bfs_emit(const BfsOut &o, BfsAlloc &al, uint64_t ci, uint32_t s, const BfsResult &r, const BfsStore &st) {
    const int lane = lane_id();
    // what the host replay needs: seen[] when an exit was found, the cycle set otherwise
    const bool want_seen = r.outcome != PF_BFS_NONE;
    const uint32_t n_list = want_seen ? r.n_seen : (r.flag_cycle ? r.n_cyc : 0);
    const uint32_t *src = want_seen ? st.ent : st.cyc;
    unsigned long long off = 0;
    if (n_list) {
        if (n_list > al.end - al.cur) {
            const uint32_t want = n_list > BFS_POOL_CHUNK ? n_list : BFS_POOL_CHUNK;
            unsigned long long got = 0;
            if (lane == 0) got = atomicAdd(o.pool_head, (unsigned long long)want);
            got = ((unsigned long long)__shfl((uint32_t)(got >> 32), 0, WAVE) << 32) | __shfl((uint32_t)got, 0, WAVE);
            al.cur = got;
            al.end = got + want;
        }
        off = al.cur;
        al.cur += n_list;
    }
    if (off + n_list <= o.pool_cap)
        for (uint32_t i = lane; i < n_list; i += WAVE) o.pool[off + i] = src[i];
    if (lane == 0) {
        pf_bfs_record rec;
        rec.entrance = s;
        rec.exit = r.exit_ov;
        rec.n_seen = r.n_seen;
        rec.n_list = n_list;
        rec.list_off = off;
        rec.outcome = r.outcome;
        rec.flag_cycle = r.flag_cycle;
        rec.flag_tip = r.flag_tip;
        rec.strict = r.strict;
        rec.pad_ = 0;
        o.rec[ci] = rec;
    }
}

// thread tier (pf_bfs.hpp): one thread per candidate; what outgrows its 8-entry tables is listed for the wavefront tier
__global__ __launch_bounds__(256) void k_bfs_thread(const uint32_t *__restrict__ succ, const uint32_t *__restrict__ pred,
                                                    const uint32_t *__restrict__ cand, uint64_t c0, uint64_t c1, BfsOut o, uint32_t *wave_list,
                                                    unsigned int *n_wave_list) {
    __shared__ uint32_t s_ent[BFS_THREAD_CAP * 256];
    __shared__ uint32_t s_todo[BFS_THREAD_CAP * 256];
    __shared__ uint32_t s_cyc[BFS_THREAD_CAP * 256];
    __shared__ uint8_t s_meta[BFS_THREAD_CAP * 256];
    const uint32_t tid = threadIdx.x;
    const BfsThreadStore st{s_ent + tid, s_todo + tid, s_cyc + tid, s_meta + tid, 256};
    const uint64_t c = c0 + (uint64_t)blockIdx.x * 256 + tid;
    const int lane = lane_id();
    const bool active = c < c1;
    BfsResult r;
    r.overflow = false;
    r.outcome = PF_BFS_NONE;
    r.n_seen = r.n_cyc = 0;
    r.flag_cycle = 0;
    uint32_t s = 0;
    if (active) {
        s = cand[c];
        r = bfs_traverse_thread(succ, pred, st, s);
    }
    const bool done = active && !r.overflow;
    // vertex lists: one atomic per wavefront for the space of all its lists
    const bool want_seen = r.outcome != PF_BFS_NONE;
    const uint32_t n_list = done ? (want_seen ? r.n_seen : (r.flag_cycle ? r.n_cyc : 0)) : 0;
    uint32_t incl = n_list;
    for (int d = 1; d < WAVE; d <<= 1) {
        const uint32_t x = __shfl_up(incl, d, WAVE);
        if (lane >= d) incl += x;
    }
    const uint32_t total = __shfl(incl, WAVE - 1, WAVE);
    unsigned long long base = 0;
    if (total) {
        if (lane == 0) base = atomicAdd(o.pool_head, (unsigned long long)total);
        base = ((unsigned long long)__shfl((uint32_t)(base >> 32), 0, WAVE) << 32) | __shfl((uint32_t)base, 0, WAVE);
    }
    const unsigned long long off = base + (incl - n_list);
    if (done) {
        if (off + n_list <= o.pool_cap)
            for (uint32_t i = 0; i < n_list; ++i) o.pool[off + i] = want_seen ? st.E(i) : st.C(i);
        pf_bfs_record rec;
        rec.entrance = s;
        rec.exit = r.exit_ov;
        rec.n_seen = r.n_seen;
        rec.n_list = n_list;
        rec.list_off = n_list ? off : 0;
        rec.outcome = r.outcome;
        rec.flag_cycle = r.flag_cycle;
        rec.flag_tip = r.flag_tip;
        rec.strict = r.strict;
        rec.pad_ = 0;
        o.rec[c - c0] = rec;
    }
    // the rest goes to the wavefront tier, in candidate order within the wavefront
    const bool over = active && r.overflow;
    const unsigned long long m = __ballot(over);
    if (m) {
        unsigned int b = 0;
        if (lane == 0) b = atomicAdd(n_wave_list, (unsigned int)__popcll(m));
        b = __shfl(b, 0, WAVE);
        if (over) wave_list[b + (unsigned int)__popcll(m & ((1ull << lane) - 1))] = (uint32_t)(c - c0);
    }
}

// wavefront tier: candidates c0 + [0, c1 - c0), or, with a list, the candidates c0 + list[0 .. *n_list)
__global__ __launch_bounds__(256) void k_bfs(const uint32_t *__restrict__ succ, const uint32_t *__restrict__ pred,
                                             const uint32_t *__restrict__ cand, uint64_t c0, uint64_t c1, BfsOut o,
                                             const uint32_t *__restrict__ list, const unsigned int *__restrict__ n_list, uint32_t cap) {
    __shared__ uint32_t s_ent[4][BFS_LDS_CAP];
    __shared__ uint32_t s_todo[4][BFS_LDS_CAP];
    __shared__ uint32_t s_cyc[4][BFS_LDS_CAP];
    __shared__ uint8_t s_meta[4][BFS_LDS_CAP];
    const int wv = threadIdx.x >> 6;
    BfsStore st{s_ent[wv], s_meta[wv], s_todo[wv], s_cyc[wv], cap};   // cap <= BFS_LDS_CAP: where this tier gives a traversal up
    st.live = o.live; st.n_live = o.n_live; st.live_cap = o.live_cap; st.hint_at = o.hint_at;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    BfsAlloc al;
    const uint64_t n_items = list ? (uint64_t)*n_list : c1 - c0;
    for (uint64_t it = wave; it < n_items; it += n_waves) {
        const uint64_t c = c0 + (list ? (uint64_t)list[it] : it);
        const uint32_t s = cand[c];
        st.hint_tag = (uint32_t)(c - c0 + 1);
        BfsResult r = bfs_traverse(succ, pred, st, s);
        if (r.overflow) {
            if (lane_id() == 0) {
                pf_bfs_record rec;
                memset(&rec, 0, sizeof(rec));
                rec.entrance = s;
                rec.exit = NONE;
                rec.outcome = BFS_DEFERRED;
                o.rec[c - c0] = rec;
                const unsigned int d = atomicAdd(o.n_deferred, 1u);
                o.deferred[d] = (uint32_t)(c - c0);
                if (o.live && !r.hinted) {   // (a table other than the seen list ran over before the notice went out)
                    const unsigned int l = atomicAdd(o.n_live, 1u);
                    if (l < o.live_cap)
                        __hip_atomic_store(&o.live[l], ((unsigned long long)s << 32) | (unsigned long long)(c - c0 + 1), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
                }
            }
        } else {
            bfs_emit(o, al, c - c0, s, r, st);
        }
        wave_sync();
    }
}

// K-BFS, big tier: same traversal over per-wave global scratch (BFS_BIG_CAP entries per table).
__global__ __launch_bounds__(64) void k_bfs_big(const uint32_t *__restrict__ succ, const uint32_t *__restrict__ pred,
                                                const uint32_t *__restrict__ cand, uint64_t c0, unsigned int n_deferred,
                                                uint32_t *scratch32, uint8_t *scratch8, BfsOut o) {
    const uint32_t wave = blockIdx.x;
    uint32_t *base = scratch32 + (size_t)wave * 3 * BFS_BIG_CAP;
    BfsStore st{base, scratch8 + (size_t)wave * BFS_BIG_CAP, base + BFS_BIG_CAP, base + 2 * BFS_BIG_CAP, BFS_BIG_CAP};
    BfsAlloc al;
    for (unsigned int d = wave; d < n_deferred; d += gridDim.x) {
        const uint32_t ci = o.deferred[d];
        const uint32_t s = cand[c0 + ci];
        BfsResult r = bfs_traverse(succ, pred, st, s);
        if (r.overflow) {
            if (lane_id() == 0) {
                const unsigned int d2 = atomicAdd(o.n_deferred2, 1u);
                o.deferred2[d2] = ci;
            }
        } else {
            bfs_emit(o, al, ci, s, r, st);
        }
        wave_sync();
    }
}

// K-BFS, last tier: direct-indexed state (pf_bfs_huge.hpp), one candidate per wave.
// two-hop rows for the huge tier: the predecessor rows of the four successors of every oriented vertex
__global__ void k_pred16(const uint32_t *__restrict__ succ, const uint32_t *__restrict__ pred, uint32_t n_ov,
                         uint32_t *__restrict__ pred16) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (; i < (uint64_t)n_ov * 4; i += stride) {
        const uint32_t sv = succ[i];
        uint4 row;
        row.x = row.y = row.z = row.w = NONE;
        if (sv != NONE) row = *reinterpret_cast<const uint4 *>(pred + (size_t)sv * 4);
        *reinterpret_cast<uint4 *>(pred16 + i * 4) = row;
    }
}

__global__ __launch_bounds__(64) void k_bfs_huge(const uint32_t *__restrict__ succ, const uint32_t *__restrict__ pred,
                                                 const uint32_t *__restrict__ cand, uint64_t c0, unsigned int n_deferred2,
                                                 uint32_t *scratch, uint32_t n_unitigs, BfsOut o) {
    const uint32_t wave = blockIdx.x;
    const size_t N = n_unitigs;
    uint32_t *b = scratch + (size_t)wave * (9 * N + 16);
    HugeStore st{b, b + N, b + 2 * N, b + 4 * N, b + 5 * N + 4, b + 7 * N + 12, n_unitigs};
    BfsStore view{st.seen, nullptr, st.todo, st.cyc, n_unitigs};
    BfsAlloc al;
    uint32_t epoch = 0;
    for (unsigned int d = wave; d < n_deferred2; d += gridDim.x) {
        const uint32_t ci = o.deferred2[d];
        const uint32_t s = cand[c0 + ci];
        ++epoch;
        BfsResult r = bfs_traverse_huge(succ, pred, st, epoch, s);
        if (r.overflow) {
            if (lane_id() == 0) o.rec[ci].outcome = BFS_TOO_LARGE;
        } else {
            bfs_emit(o, al, ci, s, r, view);
        }
        wave_sync();
    }
}

// ------------------------------------------------------------------------------------------
// host side: one driver behind the entry points
// ------------------------------------------------------------------------------------------
namespace {

// What a call delivers, said once by its entry point.
//   ON_DEVICE      records and pool are device memory and stay there
//   TO_HOST        records and pool are host memory, filled before the call returns
//   TO_HOST_ASYNC  ... filled by a copy the call starts and pf_bfs_candidates_end finishes
enum class Deliver { ON_DEVICE, TO_HOST, TO_HOST_ASYNC };
// What the wavefront tier gives up
//   ON_DEVICE  runs on the big tier, then the huge tier
//   BY_CALLER  is handed to the caller: `deferred` (and `deferred_entrance`), and the live list when it is armed
enum class LongWalks { ON_DEVICE, BY_CALLER };
struct BfsMode { Deliver deliver; LongWalks long_walks; };

// an entry point's arguments (the last line: LongWalks::BY_CALLER only, deferred_entrance optional)
struct BfsRequest {
    BfsMode mode;
    uint32_t u0, u1;
    pf_bfs_record *records; uint64_t rec_cap;
    uint32_t *pool; uint64_t pool_cap;
    uint64_t *n_records, *pool_used;
    uint32_t *deferred, *deferred_entrance; uint64_t deferred_cap, *n_deferred;
};

// the counters the kernels of one call share (BfsOut points into this block)
struct BfsCounters {
    unsigned long long pool_head;   // vertex-pool entries asked for
    unsigned int n_deferred;        // traversals the wavefront tier gave up
    unsigned int n_deferred2;       // ... and the big tier
    unsigned int n_wave_list;       // candidates the thread tier passed on to the wavefront tier
    unsigned int n_live;            // entries of the live list
};

// what the steps of one call share: candidates c0 + [0, n), the kernels' argument block, the device buffers behind it
struct BfsPlan {
    uint64_t c0, c1, n;
    BfsOut o;
    BfsCounters *d_cnt; uint32_t *d_wlist;
};

void cand_range(const pf_ctx *ctx, uint32_t u0, uint32_t u1, uint64_t *c0, uint64_t *c1) {
    const auto &v = ctx->h_cand;
    *c0 = std::lower_bound(v.begin(), v.end(), u0 * 2) - v.begin();
    *c1 = std::lower_bound(v.begin(), v.end(), u1 * 2) - v.begin();
}

// (PF_BFS_HINT_AT, read per call: measurements; beyond the tier's tables = notice only when it gives up)
uint32_t env_hint_at() { const char *e = getenv("PF_BFS_HINT_AT"); return e ? (uint32_t)std::max(9, atoi(e)) : 48u; }
// (PF_BFS_WAVE_CAP, read per call: measurements of where the wavefront tier should give up)
uint32_t env_wave_cap() { const char *e = getenv("PF_BFS_WAVE_CAP"); return e ? (uint32_t)std::max(16, std::min((int)BFS_LDS_CAP, atoi(e))) : BFS_LDS_CAP; }

// "this entry point fills host records"
int want_host_records(pf_ctx *ctx, const void *records, const char *entry_point) {
    if (!ctx || !is_device_ptr(records)) return PF_OK;
    pf::CtxErr{ctx} = std::string(entry_point) + " fills host records";
    return PF_ERR_ARG;
}

// the records the caller fills: entrance set, no exit, everything else empty
void mark_deferred(const pf_ctx *ctx, pf_bfs_record *records, uint64_t c0, const uint32_t *deferred, uint64_t n_deferred) {
    for (uint64_t d = 0; d < n_deferred; ++d) {
        pf_bfs_record &r = records[deferred[d]];
        memset(&r, 0, sizeof r);
        r.entrance = ctx->h_cand[c0 + deferred[d]];
        r.exit = NONE;
    }
}

// sizing and workspaces.  PF_OK with p.n == 0: nothing to traverse
int bfs_plan(pf_ctx *ctx, const BfsRequest &q, BfsPlan &p) {
    cand_range(ctx, q.u0, q.u1, &p.c0, &p.c1);
    const uint64_t n = p.n = p.c1 - p.c0;
    *q.n_records = n; *q.pool_used = 0;
    if (n > q.rec_cap) { pf::CtxErr{ctx} = "record buffer too small"; return PF_ERR_OVERFLOW; }
    if (n == 0) return PF_OK;
    pf_bfs_record *d_rec = q.records; uint32_t *d_pool = q.pool;
    if (q.mode.deliver != Deliver::ON_DEVICE) {
        d_rec = (pf_bfs_record *)ctx_ws(ctx, WS_BFS_REC, n * sizeof(pf_bfs_record));
        d_pool = (uint32_t *)ctx_ws(ctx, WS_BFS_POOL, (q.pool_cap ? q.pool_cap : 1) * 4);
    }
    BfsCounters *c = p.d_cnt = (BfsCounters *)ctx_ws(ctx, WS_BFS_SMALL, sizeof(BfsCounters));
    uint32_t *d_def = (uint32_t *)ctx_ws(ctx, WS_BFS_DEF, (n * 2 + 8) * 4);   // both tiers' lists
    p.d_wlist = (uint32_t *)ctx_ws(ctx, WS_BFS_WLIST, (n + 8) * 4);
    if (!d_rec || !d_pool || !c || !d_def || !p.d_wlist) return PF_ERR_HIP;
    PF_HIP(hipMemsetAsync(c, 0, sizeof(BfsCounters), ctx->stream));
    p.o = BfsOut{d_rec, d_pool, q.pool_cap, &c->pool_head, d_def, &c->n_deferred, d_def + n + 4, &c->n_deferred2, nullptr, 0, &c->n_live, 0};
    return PF_OK;
}

// the live list (armed by pf_bfs_live_deferred: the caller polls it while the kernels run) takes the notices of this call
void bfs_arm_live(pf_ctx *ctx, const BfsRequest &q, BfsPlan &p) {
    ctx->bfs_live_n = 0;
    if (!ctx->h_live || q.mode.long_walks != LongWalks::BY_CALLER) return;
    // The list is zeroed by pf_bfs_live_deferred -- once per arming, BEFORE the caller starts the threads that poll it.  Zeroing it
    // here would race with them (they would see the entries of the pass before first), and a retry after a pool overflow would wipe
    // what they are reading.  A retry writes the list again from slot 0: an entry a poller took before and the one that replaces
    // it are both real candidates of this graph, walks are keyed by (candidate, entrance), what no poller saw is walked afterwards.
    p.o.live = ctx->h_live; p.o.live_cap = (uint32_t)ctx->live_cap; p.o.hint_at = env_hint_at();
}

int bfs_read_counters(pf_ctx *ctx, const BfsPlan &p, BfsCounters &cnt) {
    PF_HIP(hipMemcpyAsync(&cnt, p.d_cnt, sizeof cnt, hipMemcpyDeviceToHost, ctx->stream));
    PF_HIP(hipStreamSynchronize(ctx->stream));
    return PF_OK;
}

// thread tier (one thread per candidate, 8-entry tables), then the wavefront tier for what outgrew it
int bfs_short_tiers(pf_ctx *ctx, const BfsPlan &p, BfsCounters &cnt) {
    ctx_begin(ctx, PF_K_BFS_THREAD);
    k_bfs_thread<<<(unsigned)((p.n + 255) / 256), 256, 0, ctx->stream>>>(ctx->d_succ, ctx->d_pred, ctx->d_cand, p.c0, p.c1, p.o, p.d_wlist, &p.d_cnt->n_wave_list);
    ctx_end(ctx);
    ctx_begin(ctx, PF_K_BFS);
    k_bfs<<<ctx_grid(ctx, (p.n / 4 + 64) * 64, 256, 8), 256, 0, ctx->stream>>>(ctx->d_succ, ctx->d_pred, ctx->d_cand, p.c0, p.c1, p.o, p.d_wlist, &p.d_cnt->n_wave_list, env_wave_cap());
    ctx_end(ctx);
    if (const int st = bfs_read_counters(ctx, p, cnt)) return st;
    ctx->bfs_live_n = cnt.n_live;
    ctx_units(ctx, PF_K_BFS, cnt.n_wave_list);
    ctx_units(ctx, PF_K_BFS_THREAD, p.n);
    return PF_OK;
}

// the long traversals on the device: the big tier, then the huge tier for what outgrew that.  Both allocate from the pool: `cnt`
// is read again behind each
int bfs_long_tiers(pf_ctx *ctx, const BfsPlan &p, BfsCounters &cnt) {
    const unsigned int waves = std::min<unsigned int>(cnt.n_deferred, 256);
    DevTmp<uint32_t> sc32; DevTmp<uint8_t> sc8;
    PF_HIP(sc32.alloc((size_t)waves * 3 * BFS_BIG_CAP * 4));
    PF_HIP(sc8.alloc((size_t)waves * BFS_BIG_CAP));
    ctx_begin(ctx, PF_K_BFS_BIG);
    k_bfs_big<<<waves, 64, 0, ctx->stream>>>(ctx->d_succ, ctx->d_pred, ctx->d_cand, p.c0, cnt.n_deferred, sc32.p, sc8.p, p.o);
    ctx_end(ctx);
    const int st = bfs_read_counters(ctx, p, cnt);
    if (st != PF_OK || cnt.n_deferred2 == 0) return st;
    // one wave per traversal, as many side by side as ~16 GiB of state allow
    const unsigned int hw = (unsigned int)std::max<size_t>(1, std::min<size_t>(std::min<size_t>(cnt.n_deferred2, 64), (16ull << 30) / (36 * (size_t)ctx->N + 64)));
    const size_t per = 9 * (size_t)ctx->N + 16;
    DevTmp<uint32_t> hs;
    PF_HIP(hs.alloc(per * hw * 4));
    PF_HIP(hipMemsetAsync(hs.p, 0, per * hw * 4, ctx->stream));
    ctx_begin(ctx, PF_K_BFS_BIG);
    if (!ctx->d_pred16) {
        PF_HIP(hipMalloc(&ctx->d_pred16, (size_t)ctx->N * 2 * 16 * 4));
        k_pred16<<<ctx_grid(ctx, (uint64_t)ctx->N * 8, 256, 8), 256, 0, ctx->stream>>>(ctx->d_succ, ctx->d_pred, ctx->N * 2, ctx->d_pred16);
    }
    k_bfs_huge<<<hw, 64, 0, ctx->stream>>>(ctx->d_succ, ctx->d_pred16, ctx->d_cand, p.c0, cnt.n_deferred2, hs.p, ctx->N, p.o);
    ctx_end(ctx);
    return bfs_read_counters(ctx, p, cnt);
}

// K-CC and the device-side commits read the records and the pool of the last call where they lie on the device
void bfs_publish(pf_ctx *ctx, const BfsRequest &q, const BfsPlan &p) {
    ctx->bfs_last_rec = p.o.rec; ctx->bfs_last_pool = p.o.pool; ctx->bfs_last_n = p.n; ctx->bfs_last_pool_len = q.pool_cap;
    ctx->bfs_call_id++;
}

// records and pool to where the entry point wants them, the entrances of the deferred candidates to the caller that asked
int bfs_deliver(pf_ctx *ctx, const BfsRequest &q, const BfsPlan &p, uint64_t pool_used) {
    const uint64_t n_deferred = q.n_deferred ? *q.n_deferred : 0;
    const size_t rec_bytes = p.n * sizeof(pf_bfs_record), pool_bytes = (size_t)pool_used * 4;
    if (q.mode.deliver == Deliver::TO_HOST) {
        PF_HIP(hipMemcpy(q.records, p.o.rec, rec_bytes, hipMemcpyDeviceToHost));
        PF_HIP(hipMemcpy(q.pool, p.o.pool, pool_bytes, hipMemcpyDeviceToHost));
        mark_deferred(ctx, q.records, p.c0, q.deferred, n_deferred);
        if (std::any_of(q.records, q.records + p.n, [](const pf_bfs_record &r) { return r.outcome == BFS_TOO_LARGE; })) {
            pf::CtxErr{ctx} = "a traversal exceeded the direct-indexed tier (internal limit)";
            return PF_ERR_OVERFLOW;
        }
    } else if (q.mode.deliver == Deliver::TO_HOST_ASYNC) {   // pf_bfs_candidates_end waits for the copies and marks the deferred records
        if (!ctx->copy_stream) PF_HIP(hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
        PF_HIP(hipMemcpyAsync(q.records, p.o.rec, rec_bytes, hipMemcpyDeviceToHost, ctx->copy_stream));
        PF_HIP(hipMemcpyAsync(q.pool, p.o.pool, pool_bytes, hipMemcpyDeviceToHost, ctx->copy_stream));
        ctx->bfs_pending.active = true; ctx->bfs_pending.records = q.records; ctx->bfs_pending.c0 = p.c0;
        ctx->bfs_pending.deferred.assign(q.deferred, q.deferred + n_deferred);
    }
    if (q.deferred_entrance) for (uint64_t d = 0; d < n_deferred; ++d) q.deferred_entrance[d] = ctx->h_cand[p.c0 + q.deferred[d]];
    return PF_OK;
}

// One K-BFS call.  A buffer of the caller's that is too small (PF_ERR_OVERFLOW) does not end the call: it goes on to tell every
// size needed, and delivers nothing.
int bfs_run(pf_ctx *ctx, const BfsRequest &q) {
    if (!ctx || !ctx->has_adj || q.u0 > q.u1 || q.u1 > ctx->N || !q.records || !q.pool || !q.n_records || !q.pool_used) return PF_ERR_ARG;
    if (ctx->bfs_pending.active) { pf::CtxErr{ctx} = "pf_bfs_candidates_end first"; return PF_ERR_ARG; }
    if (q.n_deferred) *q.n_deferred = 0;
    PF_HIP(hipSetDevice(ctx->device));
    BfsPlan p; BfsCounters cnt;
    int st = bfs_plan(ctx, q, p), status = PF_OK;
    if (st != PF_OK || p.n == 0) return st;
    bfs_arm_live(ctx, q, p);
    if ((st = bfs_short_tiers(ctx, p, cnt)) != PF_OK) return st;
    if (cnt.n_deferred && q.mode.long_walks == LongWalks::BY_CALLER) {
        // the caller walks everything that outgrew the wavefront tier itself (a host core needs ~20 ns per vertex; the 4096-entry
        // tier searches its tables linearly and is quadratic in the traversal's size)
        *q.n_deferred = cnt.n_deferred;
        if (cnt.n_deferred > q.deferred_cap) { pf::CtxErr{ctx} = "deferred-candidate buffer too small"; status = PF_ERR_OVERFLOW; }
        else PF_HIP(hipMemcpy(q.deferred, p.o.deferred, (size_t)cnt.n_deferred * 4, hipMemcpyDeviceToHost));
    } else if (cnt.n_deferred) {
        if ((st = bfs_long_tiers(ctx, p, cnt)) != PF_OK) return st;
    }
    bfs_publish(ctx, q, p);
    *q.pool_used = cnt.pool_head;
    if (cnt.pool_head > q.pool_cap) { pf::CtxErr{ctx} = "vertex pool too small"; status = PF_ERR_OVERFLOW; }
    return status == PF_OK ? bfs_deliver(ctx, q, p, cnt.pool_head) : status;
}

}  // namespace

extern "C" {

int pf_count_candidates(pf_ctx *ctx, uint32_t u0, uint32_t u1, uint64_t *n) {
    if (!ctx || !ctx->has_adj || u0 > u1 || u1 > ctx->N || !n) return PF_ERR_ARG;
    uint64_t c0, c1;
    cand_range(ctx, u0, u1, &c0, &c1);
    *n = c1 - c0;
    return PF_OK;
}

int pf_bfs_candidates(pf_ctx *ctx, uint32_t u0, uint32_t u1, pf_bfs_record *records, uint64_t rec_cap, uint32_t *pool,
                      uint64_t pool_cap, uint64_t *n_records, uint64_t *pool_used) {
    return bfs_run(ctx, {{is_device_ptr(records) ? Deliver::ON_DEVICE : Deliver::TO_HOST, LongWalks::ON_DEVICE}, u0, u1, records, rec_cap, pool, pool_cap,
                         n_records, pool_used, nullptr, nullptr, 0, nullptr});
}

int pf_bfs_candidates_split(pf_ctx *ctx, uint32_t u0, uint32_t u1, pf_bfs_record *records, uint64_t rec_cap, uint32_t *pool,
                            uint64_t pool_cap, uint64_t *n_records, uint64_t *pool_used, uint32_t *deferred, uint64_t deferred_cap,
                            uint64_t *n_deferred) {
    if (!deferred || !n_deferred) return PF_ERR_ARG;
    if (want_host_records(ctx, records, "pf_bfs_candidates_split")) return PF_ERR_ARG;
    return bfs_run(ctx, {{Deliver::TO_HOST, LongWalks::BY_CALLER}, u0, u1, records, rec_cap, pool, pool_cap, n_records, pool_used,
                         deferred, nullptr, deferred_cap, n_deferred});
}

int pf_bfs_candidates_begin(pf_ctx *ctx, uint32_t u0, uint32_t u1, pf_bfs_record *records, uint64_t rec_cap, uint32_t *pool,
                            uint64_t pool_cap, uint64_t *n_records, uint64_t *pool_used, uint32_t *deferred, uint32_t *deferred_entrance,
                            uint64_t deferred_cap, uint64_t *n_deferred) {
    if (!deferred || !deferred_entrance || !n_deferred) return PF_ERR_ARG;
    if (want_host_records(ctx, records, "pf_bfs_candidates_begin")) return PF_ERR_ARG;
    return bfs_run(ctx, {{Deliver::TO_HOST_ASYNC, LongWalks::BY_CALLER}, u0, u1, records, rec_cap, pool, pool_cap, n_records, pool_used,
                         deferred, deferred_entrance, deferred_cap, n_deferred});
}

int pf_bfs_candidates_end(pf_ctx *ctx) {
    if (!ctx) return PF_ERR_ARG;
    auto &pending = ctx->bfs_pending;
    if (!pending.active) return PF_OK;
    pending.active = false;
    PF_HIP(hipSetDevice(ctx->device));
    PF_HIP(hipStreamSynchronize(ctx->copy_stream));
    mark_deferred(ctx, pending.records, pending.c0, pending.deferred.data(), pending.deferred.size());
    return PF_OK;
}

// K-BFS with records and vertex pool left in the context's own device buffers (for K-CC and the device-side commits): nothing
// travels to the host but the deferred candidates' indices and entrances.
int pf_bfs_candidates_resident(pf_ctx *ctx, uint32_t u0, uint32_t u1, uint64_t *n_records, uint64_t *pool_used, uint32_t *deferred,
                               uint32_t *deferred_entrance, uint64_t deferred_cap, uint64_t *n_deferred) {
    if (!ctx || !n_records || !pool_used || !deferred || !deferred_entrance || !n_deferred || !ctx->has_adj || u0 > u1 || u1 > ctx->N) return PF_ERR_ARG;
    uint64_t c0, c1;
    cand_range(ctx, u0, u1, &c0, &c1);
    const uint64_t n = c1 - c0;
    uint64_t cap = std::max<uint64_t>(ctx->bfs_res_pool_cap, n * 6 + (1u << 20));
    for (int attempt = 0; attempt < 4; ++attempt) {
        pf_bfs_record *d_rec = (pf_bfs_record *)ctx_ws(ctx, WS_BFS_RES_REC, (n + 1) * sizeof(pf_bfs_record));
        uint32_t *d_pool = (uint32_t *)ctx_ws(ctx, WS_BFS_RES_POOL, (cap + 1) * 4);
        if (!d_rec || !d_pool) return PF_ERR_HIP;
        const int st = bfs_run(ctx, {{Deliver::ON_DEVICE, LongWalks::BY_CALLER}, u0, u1, d_rec, n + 1, d_pool, cap, n_records, pool_used,
                                     deferred, deferred_entrance, deferred_cap, n_deferred});
        if (st == PF_ERR_OVERFLOW && *pool_used > cap) { cap = *pool_used + *pool_used / 8 + 1024; continue; }
        if (st == PF_OK) ctx->bfs_res_pool_cap = cap;
        return st;
    }
    pf::CtxErr{ctx} = "pf_bfs_candidates_resident: the vertex pool does not converge";
    return PF_ERR_OVERFLOW;
}

int pf_bfs_live_count(pf_ctx *ctx, uint64_t *n) {
    if (!ctx || !n) return PF_ERR_ARG;
    *n = ctx->bfs_live_n;
    return PF_OK;
}

int pf_bfs_live_deferred(pf_ctx *ctx, uint64_t cap, volatile uint64_t **list) {
    if (!ctx || !list) return PF_ERR_ARG;
    *list = nullptr;
    PF_HIP(hipSetDevice(ctx->device));
    if (ctx->h_live && ctx->live_cap != cap) { (void)hipHostFree(ctx->h_live); ctx->h_live = nullptr; ctx->live_cap = 0; }
    if (cap == 0) return PF_OK;   // off
    if (!ctx->h_live) {
        void *p = nullptr;
        if (hipHostMalloc(&p, cap * 8, hipHostMallocCoherent | hipHostMallocMapped) != hipSuccess) { (void)hipGetLastError(); pf::CtxErr{ctx} = "pf_bfs_live_deferred: no pinned host memory"; return PF_ERR_HIP; }
        ctx->h_live = static_cast<unsigned long long *>(p);
        ctx->live_cap = cap;
    }
    for (uint64_t x = 0; x < cap; ++x) __atomic_store_n(&ctx->h_live[x], 0ull, __ATOMIC_RELAXED);   // (per arming: see bfs_arm_live)
    __atomic_thread_fence(__ATOMIC_SEQ_CST);
    *list = reinterpret_cast<volatile uint64_t *>(ctx->h_live);
    return PF_OK;
}

}  // extern "C"
