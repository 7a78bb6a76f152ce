// Geometry of the OPQ cross-matrix kernels (csrc/qadc_opq_kernel.hip) — HIP-free, so that
// tests/cpp/opq_plan_host.cpp can check it on the CPU.
//
// M = X0^T Y is summed in blocks of kOpqBlock vectors.  A chain is one (block j, row a, column b): one float running through
// acc = fmaf(X0[i][a], Y[i][b], acc) over the block's vectors in ascending i.  A workgroup of kOpqWG lanes owns one block and one
// tile x tile window of (a, b); its lanes form a kOpqLanes x kOpqLanes grid and each owns reg x reg whole chains in registers.
// The workgroup steps through its block `stage` vectors at a time: it stages the tile's X0 columns and the gathered Y columns
// through LDS.  A chain never leaves its lane, so the order of its operations does not depend on the launch.
#pragma once
#include <cstddef>
#include <cstdint>

namespace qadc {

constexpr int kOpqBlock = 2048;            // = QADC_OPQ_BLOCK (include/qadc.h): vectors per partial sum
constexpr int kOpqWG = 256;                // lanes of a workgroup = the kernel's __launch_bounds__
constexpr int kOpqLanes = 16;              // the lanes form a 16 x 16 grid over the tile
constexpr int kOpqMaxReg = 4;              // register tile edge per lane: 1, 2 or 4 (16 chains at most)
constexpr int kOpqStage = 32;              // vectors staged per step
constexpr int kOpqMaxDim = 1024;           // the host Procrustes solve is O(dim^3) per sweep
constexpr int kOpqReduceWG = 256;          // lanes of a workgroup of the reduce kernel, one per (a, b)

struct OpqCrossPlan {
    int dim, dsub, K, code_bytes;
    int reg;               // register tile edge per lane
    int tile;              // output tile edge per workgroup = kOpqLanes * reg
    int tiles;             // tiles per edge: tiles * tile >= dim
    int stage;             // vectors per step
    size_t lds_bytes;      // 2 * stage * tile floats: the X0 window and the Y window
    uint64_t blocks;       // ceil(n / kOpqBlock)
    uint64_t grid;         // blocks * tiles * tiles workgroups, block-major
    uint64_t partial_bytes;  // blocks * dim * dim floats of scratch
    unsigned reduce_grid;  // workgroups of the reduce kernel
};

// the shapes qadc_pq_train_* admit, without their 16-bit follow-up
constexpr bool opq_shape_ok(int sq_count, int sq_bits) {
    return sq_bits == 4 ? (sq_count == 16 || sq_count == 32) : sq_bits == 8 ? (sq_count == 4 || sq_count == 8 || sq_count == 16) : false;
}

// false: arguments the kernels do not take (the caller refuses them)
inline bool opq_cross_plan(int dim, int sq_count, int sq_bits, uint64_t n, OpqCrossPlan* p) {
    if (!opq_shape_ok(sq_count, sq_bits) || dim <= 0 || dim > kOpqMaxDim || dim % sq_count != 0) return false;
    if (n == 0 || n >= (1ull << 32)) return false;
    p->dim = dim;
    p->dsub = dim / sq_count;
    p->K = 1 << sq_bits;
    p->code_bytes = sq_bits == 4 ? sq_count / 2 : sq_count;
    p->reg = dim <= kOpqLanes ? 1 : dim <= 2 * kOpqLanes ? 2 : kOpqMaxReg;
    p->tile = kOpqLanes * p->reg;
    p->tiles = (dim + p->tile - 1) / p->tile;
    p->stage = kOpqStage;
    p->lds_bytes = (size_t)2 * p->stage * p->tile * sizeof(float);
    p->blocks = (n + kOpqBlock - 1) / kOpqBlock;
    p->grid = p->blocks * (uint64_t)(p->tiles * p->tiles);
    p->partial_bytes = p->blocks * (uint64_t)dim * (uint64_t)dim * sizeof(float);
    p->reduce_grid = (unsigned)((dim * dim + kOpqReduceWG - 1) / kOpqReduceWG);
    return p->grid < (1ull << 31) && p->lds_bytes <= 48 * 1024;
}

// The chain (a, b) that register (ra, rb) of lane `lane` of tile (ta, tb) owns — the kernel's own indexing.  A value >= dim is
// outside the matrix: the chain is not written.
constexpr int opq_cross_row(int reg, int ta, int lane, int ra) { return (ta * kOpqLanes + lane / kOpqLanes) * reg + ra; }
constexpr int opq_cross_col(int reg, int tb, int lane, int rb) { return (tb * kOpqLanes + lane % kOpqLanes) * reg + rb; }

}  // namespace qadc
