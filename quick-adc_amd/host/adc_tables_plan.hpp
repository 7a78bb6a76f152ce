// Launch geometry of the float-ADC feeders (csrc/qadc_adc_kernel.hip: adc_tables_kernel, adc_encode_kernel; DESIGN.md section
// 11) — HIP-free, so that tests/cpp/adc_tables_plan_host.cpp can check it on the CPU.  launch_adc_tables and launch_adc_encode
// launch exactly what these plans say.
//
// adc_tables_kernel: grid (query, probe group, sub-quantizer slice x centroid slice).  A workgroup holds the residuals of `probes`
// probes of one query in LDS — only the components of its `mper` sub-quantizers, plus the whole un-rotated residuals under an OPQ
// rotation — and builds `cper` blocks of 256 centroids of each of them.  Workgroup (x, y, z) covers
//   probes          [y * probes, min(ma, (y + 1) * probes))
//   sub-quantizers  [(z / cslices) * mper, (z / cslices + 1) * mper)
//   centroids       [(z % cslices) * cper * 256, (z % cslices + 1) * cper * 256)
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace qadc {
namespace adc {

constexpr int kAdcPlanMaxDim = 4096;                 // = kAdcMaxDim of csrc/qadc_adc_kernels.h (asserted where both are seen)
constexpr size_t kAdcPlanLdsBytes = 48 * 1024;       // dynamic LDS a feeder workgroup may ask for
constexpr int kAdcTablesWgFloor = 512;               // fewer workgroups than this: the launch is cut finer
constexpr int kAdcTablesWgTarget = 2048;             // the 256 centroid blocks of a 16-bit sub-quantizer are sliced up to this
constexpr int kAdcEncodeMaxGrid = 8192;              // workgroups of the 8-bit encoder; more vectors: further trips of its loop

struct AdcTablesPlan {
    int probes;        // probes of one query a workgroup holds in LDS
    int pgroups;       // probe groups = grid.y; the last may be short
    int msplit;        // sub-quantizer slices (1 or nsq)
    int mper;          // sub-quantizers per workgroup: mper * msplit == nsq
    int cper;          // blocks of 256 centroids per workgroup
    int cslices;       // centroid slices: cper * cslices * 256 == centroids
    int DS;            // the register path: the sub-vector size where it is 8, 16 or 32, else 0 (any size)
    unsigned grid_x, grid_y, grid_z;
    size_t lds_bytes;
};

// floats of dynamic LDS: res [probes][mper * ds] | vnorm [probes][mper] | (OPQ) whole [probes][dim]
inline size_t adc_tables_lds_floats(int probes, int mper, int ds, int dim, bool rotated) {
    return (size_t)probes * mper * ds + (size_t)probes * mper + (rotated ? (size_t)probes * dim : 0);
}

// false: a shape the kernel does not take (the caller refuses it); nq, ma >= 1.
inline bool adc_tables_plan(int nq, int ma, int nsq, int centroids, int dim, bool rotated, AdcTablesPlan* p) {
    if (nq <= 0 || ma <= 0 || nsq <= 0 || dim <= 0 || dim > kAdcPlanMaxDim || dim % nsq != 0 || (centroids != 256 && centroids != 65536))
        return false;
    const int ds = dim / nsq;
    // probes per workgroup: up to 16; a small batch is cut finer (sub-quantizers over grid.z, fewer probes) to fill the chip
    long groups = (ma + 15) / 16;
    int msplit = 1;
    if ((long)nq * groups < kAdcTablesWgFloor) msplit = nsq;
    if ((long)nq * groups * msplit < kAdcTablesWgFloor)
        groups = std::min<long>(ma, std::max<long>(groups, (kAdcTablesWgFloor + (long)nq * msplit - 1) / ((long)nq * msplit)));
    int probes = (int)((ma + groups - 1) / groups);
    const int mper = nsq / msplit;
    while (probes > 1 && adc_tables_lds_floats(probes, mper, ds, dim, rotated) * sizeof(float) > kAdcPlanLdsBytes) probes = (probes + 1) / 2;
    // blocks of 256 centroids per workgroup: all of them (one) for 8-bit sub-quantizers; the 256 blocks of a 16-bit one are cut
    // into slices over grid.z until the launch has about 2048 workgroups (every slice computes the residuals again)
    const long pgroups = (ma + probes - 1) / probes;
    int cper = centroids / 256;
    while (cper > 1 && (long)nq * pgroups * msplit * (centroids / (256 * cper)) < kAdcTablesWgTarget) cper /= 2;
    p->probes = probes;
    p->pgroups = (int)pgroups;
    p->msplit = msplit;
    p->mper = mper;
    p->cper = cper;
    p->cslices = centroids / (256 * cper);
    p->DS = (ds == 8 || ds == 16 || ds == 32) ? ds : 0;
    p->grid_x = (unsigned)nq;
    p->grid_y = (unsigned)pgroups;
    p->grid_z = (unsigned)(msplit * p->cslices);
    p->lds_bytes = adc_tables_lds_floats(probes, mper, ds, dim, rotated) * sizeof(float);
    return p->lds_bytes <= kAdcPlanLdsBytes && p->grid_y <= 65535u && p->grid_z <= 65535u;
}

// adc_encode_kernel: a workgroup encodes `vper` vectors at a time, chunk blockIdx.x first and every grid-th chunk after it.
// Dynamic LDS: wave keys [vper][4] u64 | wave flags [vper][4] | x [vper][dim] | ||x_m||^2 [vper][nsq] | codes [vper][nsq].
struct AdcEncodePlan {
    int vper;          // vectors per workgroup and trip
    int DS;            // as above
    unsigned grid;
    size_t lds_bytes;
};

inline bool adc_encode_plan(uint64_t n, int nsq, int dim, AdcEncodePlan* p) {
    if (n == 0 || nsq <= 0 || dim <= 0 || dim > kAdcPlanMaxDim || dim % nsq != 0) return false;
    const int ds = dim / nsq;
    p->vper = std::max(1, std::min(32, 8192 / dim));
    p->DS = (ds == 8 || ds == 16 || ds == 32) ? ds : 0;
    p->lds_bytes = (size_t)p->vper * (4 * 8 + 4 * 4 + (size_t)dim * 4 + (size_t)nsq * 4 + nsq);
    p->grid = (unsigned)std::min<uint64_t>((n + p->vper - 1) / p->vper, kAdcEncodeMaxGrid);
    return p->lds_bytes <= kAdcPlanLdsBytes;
}

}  // namespace adc
}  // namespace qadc
