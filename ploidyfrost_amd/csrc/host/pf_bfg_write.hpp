// The bytes of <sample>.bfg_colors (Bifrost's DataStorage<U>::write, format version 2, as ploidyfrost_amd/bfg_colors.py documents the
// layout) from what K-COLOR leaves: per S line its head k-mer, k-mer count and slot, and its colour set as runs of ids.  No device
// dependency: this header and ../pf_color_rule.hpp alone.
//
//   header     seven words: 2, seeds, colours, nb_cs (= lines), sz_cs (= lines + overflow), shared sets (0), overflow
//   then       the seeds; block size 1024; one {offset, 0} pair per 1024 sets; the names, a '\n' behind each; the link bits (slot in
//              use); the sets in slot order, an empty slot as the empty bit vector; the overflow triples {head k-mer left-aligned, bases, slot}
//   a set      takes the smallest form that holds it, all derived from its runs: a single id or a 61-bit vector when the largest id is
//              below 61; the run-length TinyBitmap when all ids lie in one 2^16 block and there are at most 2046 runs; otherwise a
//              Roaring bitmap of run containers.
// One known difference: the {full colours, rest} pair is never written (n_full_enc = 0 for every unitig).  Bifrost writes it only after
// its process has grown by 1 GiB while colouring, which no file can reproduce; it changes the encoding of huge inputs, not their colours.
#pragma once
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "../pf_color_rule.hpp"

namespace pf_bfg {

constexpr uint64_t FORMAT_VERSION = 2, BLOCK_SETS = 1024;
constexpr uint32_t VECTOR_IDS = 61, TINY_MAX_RUNS = 2046;

template <class T>
inline void put(std::vector<uint8_t> &out, T v) {
    const size_t at = out.size();
    out.resize(at + sizeof(T));
    memcpy(out.data() + at, &v, sizeof(T));
}

// one UnitigColors as UnitigColors::write lays it out
inline void encode_set(const pf_color::Run *runs, uint64_t n, std::vector<uint8_t> &out) {
    if (n == 0) { put<uint64_t>(out, 0x1); return; }
    const uint32_t first = runs[0].first, last = runs[n - 1].second;
    if (last < VECTOR_IDS) {
        if (n == 1 && first == last) { put<uint64_t>(out, ((uint64_t)first << 3) | 0x2); return; }
        uint64_t bits = 0;
        for (uint64_t i = 0; i < n; ++i)
            for (uint32_t v = runs[i].first; v <= runs[i].second; ++v) bits |= 1ull << v;
        put<uint64_t>(out, (bits << 3) | 0x1);
        return;
    }
    if ((first >> 16) == (last >> 16) && n <= TINY_MAX_RUNS) {   // TinyBitmap, run-length mode: header, cardinality, offset, pairs
        const uint16_t sz = (uint16_t)(2 * n + 3);
        put<uint64_t>(out, 0x0);
        put<uint16_t>(out, (uint16_t)((sz << 3) | 0x4));
        put<uint16_t>(out, (uint16_t)(2 * n));
        put<uint16_t>(out, (uint16_t)(first >> 16));
        for (uint64_t i = 0; i < n; ++i) {
            put<uint16_t>(out, (uint16_t)(runs[i].first & 0xFFFF));
            put<uint16_t>(out, (uint16_t)(runs[i].second & 0xFFFF));
        }
        return;
    }
    // Roaring portable serialisation, every 2^16 block a run container
    struct Block { uint16_t key; uint32_t card; std::vector<uint16_t> pairs; };   // pairs: start, length - 1
    std::vector<Block> blocks;
    for (uint64_t i = 0; i < n; ++i) {
        uint64_t a = runs[i].first;
        const uint64_t b = runs[i].second;
        while (a <= b) {
            const uint64_t end = std::min<uint64_t>(b, a | 0xFFFF);
            if (blocks.empty() || blocks.back().key != (uint16_t)(a >> 16)) blocks.push_back(Block{(uint16_t)(a >> 16), 0, {}});
            blocks.back().pairs.push_back((uint16_t)(a & 0xFFFF));
            blocks.back().pairs.push_back((uint16_t)(end - a));
            blocks.back().card += (uint32_t)(end - a + 1);
            a = end + 1;
        }
    }
    const uint32_t nb = (uint32_t)blocks.size();
    std::vector<uint8_t> blob;
    put<uint32_t>(blob, 12347u | ((nb - 1) << 16));
    for (uint32_t i = 0; i < (nb + 7) / 8; ++i) put<uint8_t>(blob, (uint8_t)(i * 8 + 8 <= nb ? 0xFF : (1u << (nb - i * 8)) - 1));
    for (const Block &bl : blocks) { put<uint16_t>(blob, bl.key); put<uint16_t>(blob, (uint16_t)(bl.card - 1)); }
    if (nb >= 4) {
        uint32_t pos = (uint32_t)blob.size() + 4 * nb;
        for (const Block &bl : blocks) { put<uint32_t>(blob, pos); pos += 2 + 2 * (uint32_t)bl.pairs.size(); }
    }
    for (const Block &bl : blocks) {
        put<uint16_t>(blob, (uint16_t)(bl.pairs.size() / 2));
        for (const uint16_t v : bl.pairs) put<uint16_t>(blob, v);
    }
    put<uint64_t>(out, ((uint64_t)blob.size() << 3) | 0x3);
    out.insert(out.end(), blob.begin(), blob.end());
}

// the whole file.  "" = ok, else what is wrong with the arguments
inline std::string write(const pf_color::Colored &g, int k, uint32_t n_seeds, const std::vector<std::string> &names, std::vector<uint8_t> &out) {
    const uint64_t nb_cs = g.lines.size(), sz_cs = nb_cs + g.overflow;
    if (g.run_off.size() != nb_cs + 1 || g.run_off.back() != g.runs.size()) return "the run offsets do not match the lines";
    std::vector<uint32_t> owner((size_t)sz_cs, pf_color::NO_SLOT);
    for (uint64_t j = 0; j < nb_cs; ++j) {
        const uint32_t s = g.lines[j].slot;
        if (s >= sz_cs || owner[s] != pf_color::NO_SLOT) return "line " + std::to_string(j + 1) + " has no slot of its own";
        owner[s] = (uint32_t)j;
    }
    out.clear();
    const uint64_t head[7] = {FORMAT_VERSION, n_seeds, names.size(), nb_cs, sz_cs, 0, g.overflow};
    for (const uint64_t v : head) put<uint64_t>(out, v);
    for (uint32_t s = 1; s <= n_seeds; ++s) put<uint64_t>(out, pf_color::seed_of(s));
    put<uint64_t>(out, BLOCK_SETS);
    const uint64_t n_pos = (sz_cs + BLOCK_SETS - 1) / BLOCK_SETS;
    const size_t pos_at = out.size();
    out.resize(out.size() + (size_t)n_pos * 16, 0);
    for (const std::string &nm : names) {
        out.insert(out.end(), nm.begin(), nm.end());
        out.push_back('\n');
    }
    std::vector<uint64_t> link((size_t)((sz_cs + 63) / 64), 0);
    for (uint64_t s = 0; s < sz_cs; ++s)
        if (owner[s] != pf_color::NO_SLOT) link[s >> 6] |= 1ull << (s & 63);
    for (const uint64_t w : link) put<uint64_t>(out, w);
    for (uint64_t s = 0; s < sz_cs; ++s) {
        if (s % BLOCK_SETS == 0) {   // std::streampos = {off_t, mbstate_t}
            const int64_t at = (int64_t)out.size();
            memcpy(out.data() + pos_at + (size_t)(s / BLOCK_SETS) * 16, &at, 8);
        }
        const uint32_t j = owner[s];
        if (j == pf_color::NO_SLOT) encode_set(nullptr, 0, out);
        else encode_set(g.runs.data() + g.run_off[j], g.run_off[j + 1] - g.run_off[j], out);
    }
    for (uint64_t j = 0; j < nb_cs; ++j) {
        if (g.lines[j].slot < nb_cs) continue;
        put<uint64_t>(out, pf_color::left_aligned(g.lines[j].head, k));
        put<uint64_t>(out, (uint64_t)g.lines[j].m + (uint64_t)k - 1);
        put<uint64_t>(out, g.lines[j].slot);
    }
    return "";
}

}  // namespace pf_bfg
