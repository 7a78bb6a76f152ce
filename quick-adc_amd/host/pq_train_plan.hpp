// Geometry of the PQ-training update kernel (csrc/qadc_kernels.hip: pq_train_update_kernel) — HIP-free, so
// that tests/cpp/pq_train_host.cpp can check it on the CPU.
//
// A chain is one (sub-quantizer m, centroid k, component d): one running float sum over the learning set in ascending vector
// index.  A workgroup of kPqTrainWG lanes owns up to that many chains, d fastest, and steps through the learning set `chunk`
// vectors at a time: it stages the `cols` columns its chains read, and their codes, through LDS.
//   K * dsub <  256: the chains of `mper` whole sub-quantizers (the 16-centroid shapes with short sub-vectors);
//   otherwise      : `kper` centroids of one sub-quantizer and a window of `width` <= 256 components of them.
#pragma once
#include <cstddef>
#include <cstdint>

namespace qadc {

constexpr int kPqTrainWG = 256;            // lanes of a workgroup = the kernel's __launch_bounds__
constexpr int kPqTrainChunk = 256;         // vectors per step where the staged window is at most kPqTrainStage / 256 columns wide
constexpr int kPqTrainStage = 4096;        // floats of the staged window: chunk * cols <= this (16 per lane, prefetched in registers)
constexpr int kPqTrainCodeStage = 4096;    // codes staged per step: chunk * mper <= this (16 per lane)
constexpr int kPqTrainMaxDsub = 1024;      // = the 8-bit encoder's limit: kAdcMaxDim / 4; the 4-bit one admits kPqEncodeMaxDim / 16 = 128

struct PqTrainPlan {
    int K, dsub;
    int width;      // components of one centroid a workgroup covers (min(dsub, 256))
    int dblocks;    // windows of `width` per sub-vector
    int kper;       // centroids of one sub-quantizer per workgroup
    int kblocks;
    int mper;       // sub-quantizers per workgroup (1 unless all K * dsub chains of several fit)
    int mblocks;
    int cols;       // widest staged window, in floats per vector
    int chunk;      // vectors per step
    unsigned grid;
    size_t lds_bytes;
};

// false: a shape the kernel does not take (the caller refuses it).
inline bool pq_train_plan(int sq_count, int sq_bits, int dim, PqTrainPlan* p) {
    if (sq_count <= 0 || (sq_bits != 4 && sq_bits != 8) || dim <= 0 || dim % sq_count != 0) return false;
    const int dsub = dim / sq_count, K = 1 << sq_bits;
    if (dsub > kPqTrainMaxDsub) return false;
    p->K = K;
    p->dsub = dsub;
    p->width = dsub < kPqTrainWG ? dsub : kPqTrainWG;
    p->dblocks = (dsub + p->width - 1) / p->width;
    p->kper = kPqTrainWG / p->width < K ? kPqTrainWG / p->width : K;
    p->kblocks = (K + p->kper - 1) / p->kper;
    p->mper = 1;
    if (p->kper == K && p->dblocks == 1) {
        p->mper = kPqTrainWG / (K * p->width);
        if (p->mper < 1) p->mper = 1;
        if (p->mper > sq_count) p->mper = sq_count;
    }
    p->mblocks = (sq_count + p->mper - 1) / p->mper;
    p->cols = p->mper > 1 ? p->mper * dsub : p->width;
    p->chunk = kPqTrainChunk;
    while (p->chunk * p->cols > kPqTrainStage) p->chunk /= 2;
    p->grid = (unsigned)(p->mblocks * p->kblocks * p->dblocks);
    p->lds_bytes = (size_t)p->chunk * p->cols * sizeof(float) + (size_t)p->chunk * p->mper;
    return p->chunk >= 1 && p->chunk * p->mper <= kPqTrainCodeStage && p->kper * p->width * p->mper <= kPqTrainWG &&
           p->lds_bytes <= 48 * 1024;
}

}  // namespace qadc
