// What a built graph leaves in the context until pf_unitig_release: the text of every build, and behind pf_unitig_build_colored what
// K-COLOR (pf_color.hip) colours: where every live k-mer lies in graph order, and the lines with their slots.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pf_ctx.hpp"

namespace pf {

struct UnitigState {
    char *text = nullptr;
    uint64_t bytes = 0;
    // ---- pf_unitig_build_colored only (all device arrays are owned here, but `kmers` when the caller's array was on the device) ----
    bool colored = false;
    int k = 0;
    const uint64_t *kmers = nullptr;   // the sorted distinct k-mers, n of them
    uint64_t *kmers_own = nullptr;     // the staged copy of a host array
    uint64_t n = 0, n_live = 0, n_lines = 0, longest_m = 0, overflow = 0;
    uint32_t *flat_of = nullptr;       // n entries: km_off[line] + position of k-mer i, 0xFFFFFFFF = removed
    uint64_t *heads = nullptr;         // per line: its first k-mer as written
    uint32_t *m_of = nullptr;          // per line: k-mers
    uint64_t *km_off = nullptr;        // per line: k-mers of the lines before it
    uint32_t *slot = nullptr;          // per line: its slot in the colour file
    void *color = nullptr;             // pf_color.hip: table, planes and runs, pf_color_begin .. pf_unitig_release
};

void color_destroy(UnitigState *S);   // pf_color.hip

}  // namespace pf
