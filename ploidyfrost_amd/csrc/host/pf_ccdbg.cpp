// pfh::ColoredUnitigSet and pfh::CCDBG: the colored (multi-sample) front end, reference src/CCDBG.cpp.
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <ctime>
#include <deque>
#include <mutex>
#include <set>
#include <stdexcept>
#include <thread>

#include "pf_cdbg_impl.hpp"
#include "pf_cutoffs.hpp"
#include "pf_parallel.hpp"

namespace pfh {

// ---- colored graph + CCDBG (reference src/CCDBG.cpp) -------------------------------------------------
bool ColoredUnitigSet::read(const std::string &graphfile, const std::string &colorfile, size_t nb_threads, bool verbose) {
    if (verbose) printf("ColoredCDBG::read(): Reading graph.\n");
    // abundant k-mers (unitig numbering) are decided by the CCDBG constructor with the device (K-MINZ); on the rare graph
    // whose order changes there, the colour sets are read again for the final order
    if (!graph.load_gfa(graphfile, err, true)) return false;
    if (verbose) printf("ColoredCDBG::read(): Reading colors.\n");
    colorfile_ = colorfile;
    color_threads_ = (unsigned)std::max<size_t>(nb_threads, 1);
    return colors.load(colorfile, graph, color_threads_, err);
}

bool ColoredUnitigSet::open_memory(const char *host_text, uint64_t n, const char *device_text, const uint8_t *color_bytes, uint64_t n_color_bytes,
                                   size_t nb_threads) {
    if (!graph.open_gfa_memory(host_text, n, device_text, err)) return false;
    color_bytes_ = color_bytes;
    n_color_bytes_ = n_color_bytes;
    colors_pending_ = true;
    color_threads_ = (unsigned)std::max<size_t>(nb_threads, 1);
    return true;
}

bool ColoredUnitigSet::reload_colors() {
    if (!color_bytes_) return colors.load(colorfile_, graph, color_threads_, err);
    // behind the device ingest the host holds the segment table alone: the reader asks for the packed head k-mers as load_gfa leaves them
    graph.ensure_text();
    if (graph.words.empty()) graph.pack();
    colors_pending_ = false;
    return colors.load_bytes(color_bytes_, (size_t)n_color_bytes_, graph, color_threads_, err);
}

CCDBG::CCDBG(ColoredUnitigSet &graph, const size_t &complexsize, double &m, double &d, double &g, std::string kmc_db_list,
             const size_t &thread, int device, bool quiet, std::vector<std::vector<uint64_t>> *rows_out)
    : CDBG(graph.graph, complexsize, m, d, g, device, quiet, NoCounts{}), cg_(graph) {
    if (status_ || !init_colors()) return;
    const uint32_t C = cg_.colors.n_colors;
    if (!kmc_db_list.empty()) {
        // src/CCDBG.cpp:13-43: one database name per line, one line per colour
        FILE *f = fopen(kmc_db_list.c_str(), "r");
        if (!f) { fail(PF_ERR_ARG, "CCDBG::CCDBG():Error: Open kmc database name file error"); return; }
        std::vector<std::string> names;
        {
            std::string cur;
            int ch;
            while ((ch = fgetc(f)) != EOF) {
                if (ch == '\n') { names.push_back(cur); cur.clear(); }
                else cur.push_back((char)ch);
            }
            if (!cur.empty()) names.push_back(cur);
            fclose(f);
        }
        names.resize(C);  // missing lines read as empty names, which fail to open below as in the reference
        std::vector<KmcRecords> dbs(C);
        std::vector<std::string> errs(C);
        std::vector<int> bad(C, 0);
        parallel_chunks(C, 1, (unsigned)std::max<size_t>(thread, 1), [&](size_t c, size_t, size_t) { bad[c] = !dbs[c].load(names[c], errs[c]); });
        for (uint32_t c = 0; c < C; ++c) {
            if (bad[c]) { fail(PF_ERR_ARG, "CCDBG::CCDBG():Error: Open kmc database " + names[c] + " error (" + errs[c] + ")"); return; }
            if ((int)dbs[c].k != g_.k) { fail(PF_ERR_ARG, "CCDBG::CCDBG():Error: k of kmc database " + names[c] + " differs from the graph's"); return; }
            if (!quiet_) printf("CCDBG::CCDBG(): kmc database %s initialized\n", names[c].c_str());
        }
        // every database is decoded on the device (K-KMC) from its mapped record file; the joint table is built from those arrays
        std::vector<uint64_t *> pk(C, nullptr);
        std::vector<uint32_t *> pc(C, nullptr);
        std::vector<uint64_t> n(C), mn(C), mx(C);
        std::vector<int> both(C);
        int st = PF_OK;
        if (rows_out) rows_out->assign(C, {});
        for (uint32_t c = 0; c < C && st == PF_OK; ++c) {
            st = pf_kmc_decode(ctx_, dbs[c].records, dbs[c].total, dbs[c].suffix_bytes, dbs[c].counter_size, dbs[c].lut.data(), dbs[c].n_lut(),
                               dbs[c].lut_prefix_len, dbs[c].k, &pk[c], &pc[c]);
            if (st == PF_OK && rows_out) st = kmc_rows_of_counts(ctx_, dbs[c], pc[c], (*rows_out)[c]);
            n[c] = dbs[c].total;
            mn[c] = dbs[c].min_count;
            mx[c] = dbs[c].max_count;
            both[c] = dbs[c].both_strands;
        }
        if (st == PF_OK) st = pf_upload_counts_colored(ctx_, C, pk.data(), pc.data(), n.data(), mn.data(), mx.data(), both.data());
        for (uint32_t c = 0; c < C; ++c) { pf_device_free(ctx_, pk[c]); pf_device_free(ctx_, pc[c]); }
        if (st != PF_OK) { fail(st, std::string("CCDBG::CCDBG():Error: ") + pf_last_error(ctx_)); return; }
        colours_to_device();
    }
    if (!quiet_) printf("CCDBG::CCDBG():CCDBG initialized!\n");
}

bool CCDBG::init_colors() {
    if ((cg_.colors_pending() || cg_.graph.n_abundant) && !cg_.reload_colors()) { fail(PF_ERR_ARG, "CCDBG::CCDBG():Error: " + cg_.err); return false; }
    col_ = &cg_.colors;
    st_.col = col_;
    const uint32_t C = cg_.colors.n_colors;
    if (C > PF_MAX_COLORS_TABLE) { fail(PF_ERR_ARG, "CCDBG::CCDBG():Error: more colours than the device table holds"); return false; }
    // the colour gate of the accept commit goes to the device with the graph: the commits run there (pf_replay_device).  Colour sets
    // are (C + 63) / 64 words per unitig, on the host and on the device alike: the reference has no limit on the number of colours
    // (src/CCDBG.cpp:2759-2853 loops over getNbColors()), the joined table's PF_MAX_COLORS_TABLE is the only one here.
    const int st = pf_replay_set_colours(ctx_, C, cg_.colors.full_mask.data(), cg_.colors.size_total.data(), cg_.colors.n_full_enc.data());
    colours_on_device_ = st == PF_OK;
    return true;
}

void CCDBG::colours_to_device() {
    const uint32_t C = cg_.colors.n_colors;
    int st = PF_OK;
    // the colour sets the calling phase asks about go to the device as well (pf_call_set_colours): the mask of colours on every
    // k-mer, UnitigColors::size(), and one bit per k-mer for a colour on part of a unitig
    if (const char *e = getenv("PF_CALL")) resident_ = strcmp(e, "host") != 0;
    if (resident_) {
        const ColorSets &cs = cg_.colors;
        const uint32_t N = g_.n();
        std::vector<uint32_t> us;
        us.reserve(cs.partial.size());
        for (const auto &kv : cs.partial) us.push_back(kv.first);
        std::sort(us.begin(), us.end());
        std::vector<uint32_t> part_first((size_t)N + 1, 0), part_colour;
        std::vector<uint64_t> part_word, bits;
        for (uint32_t u : us) part_first[(size_t)u + 1] = (uint32_t)cs.partial.at(u).size();
        for (uint32_t u = 0; u < N; ++u) part_first[(size_t)u + 1] += part_first[u];
        for (uint32_t u : us)
            for (const ColorSets::Partial &pt : cs.partial.at(u)) {
                part_colour.push_back(pt.colour);
                part_word.push_back(bits.size());
                bits.insert(bits.end(), pt.bits.begin(), pt.bits.end());
            }
        st = pf_call_set_colours(ctx_, C, cs.full_mask.data(), cs.size_total.data(), part_first.data(), part_colour.data(), part_word.data(), bits.data(),
                                 part_colour.size(), bits.size());
        colored_resident_ = st == PF_OK;
    }
}

CCDBG::CCDBG(ColoredUnitigSet &graph, const size_t &complexsize, double &m, double &d, double &g, const ColorCounts &counts, int device, bool quiet)
    : CDBG(graph.graph, complexsize, m, d, g, device, quiet, NoCounts{}, counts.ctx), cg_(graph) {
    if (status_ || !init_colors()) return;
    const uint32_t C = cg_.colors.n_colors;
    if (counts.kmers.size() != C || counts.counts.size() != C || counts.n.size() != C) {
        fail(PF_ERR_ARG, "CCDBG::CCDBG():Error: " + std::to_string(counts.n.size()) + " count arrays for " + std::to_string(C) + " colors");
        return;
    }
    if (counts.k != g_.k) { fail(PF_ERR_ARG, "CCDBG::CCDBG():Error: k of the counted k-mers differs from the graph's"); return; }
    const std::vector<uint64_t> mn(C, counts.min_count), mx(C, counts.max_count);
    const std::vector<int> both(C, 1);
    const int st = pf_upload_counts_colored(ctx_, C, counts.kmers.data(), counts.counts.data(), counts.n.data(), mn.data(), mx.data(), both.data());
    if (st != PF_OK) { fail(st, std::string("CCDBG::CCDBG():Error: ") + pf_last_error(ctx_)); return; }
    colours_to_device();
    if (!quiet_) printf("CCDBG::CCDBG():CCDBG initialized!\n");
}

int CCDBG::ploidyEstimation_multithread_ptr(const std::string &outpre, const std::vector<std::pair<int, int>> &cutoff, const size_t &thr) {
    return ploidy_estimation(outpre, cutoff, thr);
}

}  // namespace pfh
