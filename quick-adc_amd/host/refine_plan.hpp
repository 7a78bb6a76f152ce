// Launch geometry of exact re-ranking (csrc/qadc_refine_kernel.hip: refine_dist_kernel, refine_select_kernel; DESIGN.md section
// 11.11) — HIP-free, so that tests/cpp/refine_plan_host.cpp can check it on the CPU.  launch_refine_dist and launch_refine_select
// launch exactly what this plan says.
//
// A call runs in passes of `pass_nq` whole queries, so that the scratch of 64-bit words [pass_nq][r_in] stays bounded.
//
// refine_dist_kernel: one candidate per wave, kRefineWaves waves per workgroup.  The candidates of a pass are flattened: workgroup b
// serves query b / chunks of the pass and the candidates [c0, min(r_in, c0 + cands_per_wg)), c0 = (b % chunks) * cands_per_wg, of
// its list; wave w takes c0 + w * kRefineInFlight + k * kRefineWaves * kRefineInFlight + (0 .. kRefineInFlight - 1), k = 0, 1, ...:
// kRefineInFlight rows streamed side by side to cover the gather's latency.  Dynamic LDS: the query, dim floats.
//
// refine_select_kernel: one workgroup per query sorts sort_n >= r_in words in LDS (sort_n one of kRefineSortSizes) with
// sort_threads threads; dynamic LDS: the words, then one counter per thread for the prefix sum over the survivors' marks.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace qadc {
namespace refine {

constexpr int kRefinePlanMaxDim = 4096;
constexpr int kRefinePlanMaxIn = 8192;               // = QADC_REFINE_MAX_IN (asserted where both are seen)
constexpr int kRefineWaves = 4;                      // waves of a distance workgroup (256 threads)
constexpr int kRefineInFlight = 4;                   // candidates a wave streams side by side
constexpr int kRefineMaxCandsPerWg = 64;
constexpr int kRefineWgFloor = 1024;                 // fewer distance workgroups than this: the lists are cut finer
constexpr uint64_t kRefinePassCands = 1ull << 24;    // candidates of one pass (128 MiB of words)
constexpr size_t kRefineLdsLimit = 160 * 1024;       // LDS of a CU of gfx950
constexpr size_t kRefineLdsDefault = 64 * 1024;      // dynamic LDS a kernel may ask for without raising its limit
constexpr int kRefineSortSizes[3] = {512, 2048, 8192};

struct RefinePlan {
    int pass_nq;            // whole queries per pass
    int passes;
    int cands_per_wg;       // a multiple of kRefineInFlight
    int chunks;             // workgroups per query: ceil(r_in / cands_per_wg)
    size_t dist_lds_bytes;
    int sort_n;             // the padded sort size
    int sort_threads;
    size_t select_lds_bytes;
    // grid of the distance launch of a pass of n queries: n * chunks;  of the select launch: n
};

// false: a shape the kernels do not take (the caller refuses it)
inline bool refine_plan(int nq, int r_in, int dim, RefinePlan* p) {
    if (nq <= 0 || r_in <= 0 || r_in > kRefinePlanMaxIn || dim <= 0 || dim > kRefinePlanMaxDim) return false;
    p->pass_nq = (int)std::min<uint64_t>((uint64_t)nq, std::max<uint64_t>(1, kRefinePassCands / (uint64_t)r_in));
    p->passes = (nq + p->pass_nq - 1) / p->pass_nq;
    int cpw = kRefineMaxCandsPerWg;
    while (cpw > kRefineInFlight && (int64_t)std::min(nq, p->pass_nq) * ((r_in + cpw - 1) / cpw) < kRefineWgFloor) cpw /= 2;
    p->cands_per_wg = cpw;
    p->chunks = (r_in + cpw - 1) / cpw;
    p->dist_lds_bytes = (size_t)dim * sizeof(float);
    p->sort_n = kRefineSortSizes[2];
    for (int i = 2; i >= 0; --i)
        if (r_in <= kRefineSortSizes[i]) p->sort_n = kRefineSortSizes[i];
    p->sort_threads = std::min(1024, p->sort_n / 2);
    p->select_lds_bytes = (size_t)p->sort_n * sizeof(uint64_t) + (size_t)p->sort_threads * sizeof(uint32_t);
    return p->dist_lds_bytes <= kRefineLdsDefault && p->select_lds_bytes <= kRefineLdsLimit;
}

}  // namespace refine
}  // namespace qadc
