// What the kernels of both gzip readers (pf_inflate.hip, pf_gunzip.hip) put around the decoder of pf_inflate_core.hpp: the wavefront's
// sync, a view of bytes in memory, and the compressed bytes through a window in LDS.  Device code only; one wavefront per block.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pf {

constexpr int GZ_WAVE = 64;
constexpr uint32_t GZ_WINDOW = 1024;   // bytes of the compressed input held in LDS
constexpr uint32_t GZ_KEEP = 64;       // of them behind the byte asked for (the reader steps back by at most two)

// between the writes of some lanes and the reads of others
struct GzSync {
    __host__ __device__ void operator()() const {
#if defined(__HIP_DEVICE_COMPILE__)
        __syncthreads();
#endif
    }
};

struct GzBytes {
    const uint8_t *p;
    __device__ uint32_t operator[](uint64_t i) const { return p[i]; }
};

// p[0, n_in) through a window in LDS; every lane of the wavefront asks for the same byte at the same time.  No address outside
// p[0, n_in) is read: the refill tests every dword, and every byte of a dword that crosses an edge.
struct GzIn {
    const uint8_t *p;
    uint32_t n_in, lane;
    uint32_t *win;              // GZ_WINDOW / 4 dwords
    mutable uint32_t base;      // the window holds bytes [base - shift, base - shift + GZ_WINDOW), base a multiple of 4
    uint32_t shift;             // p's distance from the dword boundary in front of it
    // the window filled for a reader that starts at byte `first`
    __device__ GzIn(const uint8_t *bytes, uint32_t n, uint32_t lane_, uint32_t *window, uint32_t first)
        : p(bytes), n_in(n), lane(lane_), win(window), base(0u), shift((uint32_t)((uintptr_t)bytes & 3u)) {
        refill(first + shift);
    }
    __device__ void refill(uint32_t j) const {   // j = i + shift
        __syncthreads();
        base = (j >= GZ_KEEP ? j - GZ_KEEP : 0u) & ~3u;
        const uint8_t *q = p - shift;   // a dword boundary; nothing in front of p is read
        for (uint32_t k = lane; k < GZ_WINDOW / 4; k += GZ_WAVE) {
            const uint64_t jj = (uint64_t)base + 4 * k;
            uint32_t v = 0;
            if (jj >= shift && jj + 4 <= (uint64_t)shift + n_in) {
                v = *reinterpret_cast<const uint32_t *>(q + jj);
            } else {
                for (uint32_t b = 0; b < 4; ++b)
                    if (jj + b >= shift && jj + b < (uint64_t)shift + n_in) v |= (uint32_t)q[jj + b] << (8 * b);
            }
            win[k] = v;
        }
        __syncthreads();
    }
    __device__ uint8_t byte(uint32_t i) const {   // i < n_in
        const uint32_t j = i + shift;
        if (j - base >= GZ_WINDOW) refill(j);
        return reinterpret_cast<const uint8_t *>(win)[j - base];
    }
    __device__ uint8_t raw(uint32_t i) const { return p[i]; }   // i < n_in (a stored block's bytes)
};

}  // namespace pf
