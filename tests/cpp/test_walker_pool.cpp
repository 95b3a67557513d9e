// Host-only check of pfh::WalkerPool (ploidyfrost_amd/csrc/host/pf_bfs_host.hpp), the one place where findSuperBubble's host paths take
// a walker, walk and copy the list out: eight threads walk a small hand-built graph from every entrance through one pool, many
// times over; every record and list equals that of a single-threaded HugeWalker::walk, whatever the record held before, and the
// pool never holds more walkers than there were threads.  Built (with pf_bfs_host.cpp, nothing else) and run by
// tests/test_host_logic_cpu.py.
#include <atomic>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "pf_bfs_host.hpp"

namespace {
constexpr uint32_t NONE = 0xFFFFFFFFu, N = 600;
std::vector<uint32_t> succ(2 * N * 4, NONE), pred(2 * N * 4, NONE);

bool put(std::vector<uint32_t> &rows, uint32_t at, uint32_t v) {
    for (int b = 0; b < 4; ++b) {
        if (rows[at * 4 + b] == v) return false;
        if (rows[at * 4 + b] == NONE) { rows[at * 4 + b] = v; return true; }
    }
    return false;
}
bool has_room(const std::vector<uint32_t> &rows, uint32_t at, uint32_t v) {
    for (int b = 0; b < 4; ++b)
        if (rows[at * 4 + b] == v) return false;
    return rows[at * 4 + 3] == NONE;
}
// a -> b and its mirror rc(b) -> rc(a), when all four rows have room
void edge(uint32_t a, uint32_t b) {
    const uint32_t ra = a ^ 1, rb = b ^ 1;
    if (!has_room(succ, a, b) || !has_room(pred, b, a) || !has_room(succ, rb, ra) || !has_room(pred, ra, rb)) return;
    put(succ, a, b); put(pred, b, a);
    if (rb != a || ra != b) { put(succ, rb, ra); put(pred, ra, rb); }
}
}  // namespace

int main() {
    // a chain with bubbles of several shapes, tips, back edges (cycles) and strand switches
    uint32_t x = 12345;
    auto rnd = [&] { x = x * 1664525u + 1013904223u; return x >> 8; };
    for (uint32_t i = 0; i + 1 < N; ++i) {
        if (i % 29 != 11) edge(2 * i, 2 * (i + 1));
        if (i % 3 == 0 && i + 2 < N) edge(2 * i, 2 * (i + 2));
        if (i % 7 == 2 && i + 3 < N) edge(2 * i, 2 * (i + 3));
        if (i % 41 == 5 && i >= 6) edge(2 * i, 2 * (i - 6));
        if (i % 53 == 9) edge(2 * i, 2 * (rnd() % N) + 1);
        if (i % 13 == 4) edge(2 * i + 1, 2 * (rnd() % N));
    }
    struct Want {
        pf_bfs_record rec;
        std::vector<uint32_t> list;
    };
    std::vector<Want> want(2 * N);
    uint32_t outcomes[4] = {0, 0, 0, 0};
    {
        pfh::HugeWalker w;
        for (uint32_t ov = 0; ov < 2 * N; ++ov) {
            memset(&want[ov].rec, 0, sizeof(pf_bfs_record));
            const std::vector<uint32_t> &l = w.walk(succ.data(), pred.data(), N, ov, want[ov].rec);
            want[ov].list.assign(l.begin(), l.begin() + want[ov].rec.n_list);
            outcomes[want[ov].rec.outcome & 3]++;
        }
    }
    constexpr unsigned kThreads = 8, kRounds = 25;
    pfh::WalkerPool pool;
    std::atomic<long> bad{0}, walks{0};
    std::vector<std::thread> th;
    for (unsigned t = 0; t < kThreads; ++t)
        th.emplace_back([&, t] {
            std::vector<uint32_t> out;
            for (unsigned round = 0; round < kRounds; ++round)
                for (uint32_t k = 0; k < 2 * N; ++k) {
                    const uint32_t ov = (k * (2 * t + 1) + 97 * round) % (2 * N);   // every thread in an order of its own
                    pf_bfs_record r;
                    memset(&r, 0xAB, sizeof r);   // (whatever the record held before)
                    pool.walk(succ.data(), pred.data(), N, ov, r, out);
                    if (memcmp(&r, &want[ov].rec, sizeof r) != 0 || out != want[ov].list) bad++;
                    walks++;
                }
        });
    for (auto &t : th) t.join();
    const size_t at_rest = pool.size();
    if (bad || at_rest < 1 || at_rest > kThreads || walks != (long)kThreads * kRounds * 2 * N || !outcomes[0] || !(outcomes[1] + outcomes[2] + outcomes[3])) {   // (the graph has walks that end at an exit and walks that do not)
        printf("FAILED: %ld of %ld walks differ, %zu walkers in the pool, outcomes %u %u %u %u\n", bad.load(), walks.load(), at_rest, outcomes[0], outcomes[1],
               outcomes[2], outcomes[3]);
        return 1;
    }
    printf("ok\n");
    return 0;
}
