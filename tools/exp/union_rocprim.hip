// The form K-UNION is measured against (tools/bench_run_multi.py): concatenate the sets, rocprim::radix_sort_keys, rocprim::unique.
// A library of its own so that rocprim's kernels stay out of libploidyfrost_hip.so (pf_scan.hpp says why).
//   hipcc --offload-arch=gfx950 -O3 -shared -fPIC -o tools/exp/libunion_rocprim.so tools/exp/union_rocprim.hip
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <cstring>

#include <rocprim/rocprim.hpp>

#define CHECK(call) do { if ((call) != hipSuccess) return -1.0; } while (0)

// sets_dev[c]: n[c] keys on the device.  Returns the milliseconds between two events around everything (allocations included, as
// pf_kernel_time brackets pf_kmer_union), -1 on an error; *n_out = size of the union, first_keys (may be NULL): up to 4 of its keys.
extern "C" double union_rocprim_ms(const uint64_t *const *sets_dev, const uint64_t *n, uint32_t n_sets, uint64_t *n_out, uint64_t *first_keys) {
    uint64_t total = 0;
    for (uint32_t c = 0; c < n_sets; ++c) total += n[c];
    hipEvent_t a, b;
    CHECK(hipEventCreate(&a));
    CHECK(hipEventCreate(&b));
    CHECK(hipEventRecord(a, nullptr));
    uint64_t *cat = nullptr, *sorted = nullptr, *uniq = nullptr, *count = nullptr;
    void *tmp = nullptr;
    CHECK(hipMalloc(&cat, (total + 1) * 8));
    CHECK(hipMalloc(&sorted, (total + 1) * 8));
    CHECK(hipMalloc(&uniq, (total + 1) * 8));
    CHECK(hipMalloc(&count, 8));
    uint64_t at = 0;
    for (uint32_t c = 0; c < n_sets; ++c) {
        if (n[c]) CHECK(hipMemcpyAsync(cat + at, sets_dev[c], n[c] * 8, hipMemcpyDeviceToDevice, nullptr));
        at += n[c];
    }
    size_t need_sort = 0, need_uniq = 0;
    CHECK(rocprim::radix_sort_keys(nullptr, need_sort, cat, sorted, total));
    CHECK(rocprim::unique(nullptr, need_uniq, sorted, uniq, count, total));
    CHECK(hipMalloc(&tmp, (need_sort > need_uniq ? need_sort : need_uniq) + 8));
    CHECK(rocprim::radix_sort_keys(tmp, need_sort, cat, sorted, total));
    CHECK(rocprim::unique(tmp, need_uniq, sorted, uniq, count, total));
    uint64_t h = 0;
    CHECK(hipMemcpy(&h, count, 8, hipMemcpyDeviceToHost));
    CHECK(hipEventRecord(b, nullptr));
    CHECK(hipEventSynchronize(b));
    float ms = 0;
    CHECK(hipEventElapsedTime(&ms, a, b));
    if (n_out) *n_out = h;
    if (first_keys && h) CHECK(hipMemcpy(first_keys, uniq, (h < 4 ? h : 4) * 8, hipMemcpyDeviceToHost));
    (void)hipFree(cat);
    (void)hipFree(sorted);
    (void)hipFree(uniq);
    (void)hipFree(count);
    (void)hipFree(tmp);
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    return (double)ms;
}
