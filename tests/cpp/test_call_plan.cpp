// The sizing plan of the resident calling pipeline (ploidyfrost_amd/csrc/pf_call_plan.hpp) on its own, no GPU: pf_call_align_lane and
// pf_call_reserve_lanes take every grid, scratch size and first-call capacity from it, so the numbers are pinned here.  Every
// expectation is a literal worked out by hand from the expressions the two functions carried before the plan existed (e.g. complex
// size 8 -> depth max(8 + 4, 16) = 16 -> (256 * 8 + 256 * 4 + (10 * 16 + 4) * 4 = 3728, to the next 256) = 3840); none is computed by
// the code under test.
#include <cstdint>
#include <cstdio>

#include "pf_call_plan.hpp"

using namespace pf_call;

static int bad = 0;
static void eq(const char *what, uint64_t got, uint64_t want) {
    if (got != want) { fprintf(stderr, "%s: %llu, expected %llu\n", what, (unsigned long long)got, (unsigned long long)want); ++bad; }
}
#define EQ(expr, want) eq(#expr, (uint64_t)(expr), (uint64_t)(want))

static void pools(const char *what, const BatchPools &p, uint64_t path_pool, uint64_t path_text, uint64_t row_text, uint64_t sites, uint64_t groups, uint64_t ilen,
                  uint64_t walk) {
    char name[96];
    const uint64_t got[7] = {p.path_pool, p.path_text, p.row_text, p.sites, p.groups, p.ilen, p.walk}, want[7] = {path_pool, path_text, row_text, sites, groups, ilen, walk};
    const char *field[7] = {"path_pool", "path_text", "row_text", "sites", "groups", "ilen", "walk"};
    for (int x = 0; x < 7; ++x) { snprintf(name, sizeof name, "%s.%s", what, field[x]); eq(name, got[x], want[x]); }
}

int main() {
    static_assert(FIRST_ROW_TEXT == 384 && FIRST_SITES == 4 && FIRST_GROUPS == 12 && FIRST_ILEN == 2 && FIRST_PATH_TEXT == 64, "first-pass constants");
    // grids: 16, 16, 12, 4, 8 wavefronts per CU
    const CallGrids big = call_grids(256), one = call_grids(1);
    EQ(big.paths, 4096); EQ(big.sites, 4096); EQ(big.pair, 3072); EQ(big.pair2, 1024); EQ(big.stack, 2048);
    EQ(one.paths, 16); EQ(one.sites, 16); EQ(one.pair, 12); EQ(one.pair2, 4); EQ(one.stack, 8);

    // K-PATHS
    EQ(depth_cap(0), 16); EQ(depth_cap(8), 16); EQ(depth_cap(12), 16); EQ(depth_cap(13), 17); EQ(depth_cap(1000), 1004);
    EQ(paths_per_wave(16), 3840);            // 2048 + 1024 + 656 = 3728
    EQ(paths_per_wave(1004), 43264);         // 3072 + 10044 * 4 = 43248
    EQ(paths_big_per_wave(16, 65535), 787200);     // 656 + 65536 * 12 = 787088
    EQ(paths_big_per_wave(1004, 65535), 826624);   // 40176 + 786432 = 826608
    EQ(paths_big_per_wave(100, 65535), 790528);    // 4016 + 786432 = 790448
    EQ(paths_big_grid(5), 5); EQ(paths_big_grid(1000), 32);
    EQ(MANY_LIST_MIN, 4096); EQ(grown_many(5000), 5689);
    EQ(grown(1000, 1024), 2149); EQ(grown(0, 4096), 4096);

    // K-PAIR's second tier
    EQ(call_pair2_grid(100, big), 2); EQ(call_pair2_grid(1000000, big), 1024); EQ(call_pair2_grid(1, one), 1); EQ(call_pair2_grid(1000, one), 4);
    EQ(pair2_min(256), 8192); EQ(pair2_min(1), 32);

    // K-SITES: k 25 and 31, no colours and 130 (three words a set)
    EQ(first_site_string(25), 114); EQ(first_site_string(31), 126);
    EQ(grown_site_string(127), 128); EQ(grown_site_string(128), 128); EQ(grown_site_string(129), 192);
    EQ(sites_rows_cap(0), 256); EQ(sites_rows_cap(256), 256); EQ(sites_rows_cap(257), 320); EQ(sites_rows_cap(300), 320);
    EQ(sites_per_wave(256, 114, 0, 1), 64000);       // 58368 + 256 * 22
    EQ(sites_per_wave(256, 2 * 31 + 64, 0, 1), 70144);   // 64512 + 5632
    EQ(sites_per_wave(320, 126, 0, 1), 87808);       // 80640 + 7040 = 87680
    EQ(sites_per_wave(256, 126, 130, 3), 348928);    // 70144 + 256 * (48 + 1040 + 1)
    EQ(sites_per_wave(320, 114, 130, 3), 428544);    // 72960 + 7040 + 320 * 1089 = 428480
    EQ(call_sites_grid(10, big, 70144), 10); EQ(call_sites_grid(1000000, big, 70144), 4096); EQ(call_sites_grid(1000000, big, 1u << 20), 2048);
    EQ(call_sites_grid(0, big, 70144), 1); EQ(call_sites_grid(100, one, 70144), 16);
    EQ(site_values_cap(0, 1000, 1000, 0), 1033024); EQ(site_values_cap(130, 1000, 1000, 0), 2065024); EQ(site_values_cap(0, 1000, 1000, 5000000), 5000000);

    // the pools of a range: 1 bubble on one CU, 100 000 and 2^24 on 256
    const LearntPools none;
    pools("nb 1", batch_pools(1, one, none, false), 3072, 65600, 65920, 68, 76, 66, 0);
    pools("nb 1 colored", batch_pools(1, one, none, true), 3072, 65600, 65920, 68, 76, 66, 5122);
    pools("nb 100000", batch_pools(100000, big, none, true), 575312, 6465536, 38465536, 400064, 1200064, 200064, 1249600);
    pools("nb 2^24", batch_pools(1u << 24, big, none, true), 8913920, 1073807360ull, 6442516480ull, 67108928, 201326656, 33554496, 34604032);
    EQ(batch_pools(1, one, none, false).path_entries(1), 3076);
    EQ(batch_pools(100000, big, none, false).path_entries(100000), 975312);
    EQ(batch_pools(1u << 24, big, none, false).path_entries(1u << 24), 76022784);
    // what earlier batches learnt wins where it is larger, field by field
    LearntPools l;
    l.path_pool = 1000000; l.path_text = 1; l.row_text = 50000000; l.sites = 400064; l.groups = 1200065; l.ilen = 0; l.walk = 2000000;
    pools("learnt", batch_pools(100000, big, l, true), 1000000, 6465536, 50000000, 400064, 1200065, 200064, 2000000);
    pools("learnt, not colored", batch_pools(100000, big, l, false), 1000000, 6465536, 50000000, 400064, 1200065, 200064, 0);
    EQ(row_text_need(1000, 10, 100), 20280);

    // a reservation's guesses
    EQ(reserve_job_index_bytes(1), 4096); EQ(reserve_job_index_bytes(100000), 104096); EQ(reserve_job_index_bytes(100003), 104096);
    EQ(reserve_job_index_bytes(1u << 24), 16781312);
    EQ(reserve_site_values(100000, big), 4220328); EQ(reserve_site_values(1, one), 17408); EQ(reserve_site_values(100003, big), 4220328);

    if (bad) return 1;
    printf("ok\n");
    return 0;
}
