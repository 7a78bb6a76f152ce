// Geometry of the PQ decode kernels (csrc/qadc_decode_kernel.hip) — HIP-free, so that
// tests/cpp/pq_decode_plan_host.cpp can sweep it on the CPU.
//
// Without a rotation the decode is a gather bounded by the n * dim * 4 bytes it writes.  A workgroup takes `rows_per_wg` rows at a
// time: it stages their code bytes through LDS with one coalesced read (a row's code bytes are read once), then its lanes own `vec`
// consecutive components each and copy them from the codebooks.  The codebooks are staged in LDS when all of them fit beside the
// code bytes in the default dynamic limit (kDecodeLdsLimit), else they are read through the L2; at 16 bits (256 KiB per component)
// always through the L2.  The workgroups of a launch stride over the row blocks, so a staged codebook serves several blocks.
//
// With a rotation a chain is one (row i, column c): acc = fmaf(y[i][r], rotation[r][c], acc) over ascending r.  A workgroup of
// kDecodeWG lanes owns a tile x tile window of (i, c); its lanes form a kDecodeLanes x kDecodeLanes grid and each owns reg x reg
// whole chains in registers.  The workgroup walks r in windows of kDecodeStage, staging the gathered y and the rows of the rotation
// through LDS.  A chain never leaves its lane, so its order does not depend on the launch.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace qadc {

constexpr uint64_t kDecodeChunk = 262144;      // = QADC_DECODE_CHUNK (include/qadc.h): rows per pass
constexpr int kDecodeWG = 256;                 // lanes of a workgroup = every decode kernel's __launch_bounds__
constexpr int kDecodeItems = 4;                // gather: stores per lane and row block the geometry aims at
constexpr int kDecodeMaxRows = 256;            // gather: rows of a block at most (their code bytes: 4 KiB of LDS at most)
constexpr unsigned kDecodeMaxGrid = 1024;      // gather: workgroups of a launch at most (4 per CU of 256); they stride over the blocks
constexpr size_t kDecodeLdsLimit = 64 * 1024;  // dynamic LDS a launch may ask for without raising the function's limit
constexpr int kDecodeLanes = 16;               // rotation: the lanes form a 16 x 16 grid over the tile
constexpr int kDecodeMaxReg = 4;               // rotation: register tile edge per lane: 1, 2 or 4
constexpr int kDecodeStage = 32;               // rotation: components r staged per step
constexpr int kDecodeErrTile = 64;             // error: rows and columns of the staged window (one chain per row, kDecodeErrTile lanes walk)

struct PqDecodePlan {
    int dim, dsub, sq_count, sq_bits, centroids, code_bytes;
    // the gather (no rotation)
    int vec;                 // components per lane and store: 4 (16-byte stores) when dim % 4 == 0 and `out` is 16-byte aligned, else 1
    int lanes_per_row;       // dim / vec
    int rows_per_wg;         // rows of a block
    int cb_in_lds;           // 1: the codebooks are staged in LDS
    size_t cb_bytes;         // centroids * dim * 4: all codebooks
    size_t gather_lds;       // dynamic LDS of the gather: the staged codebooks (if any), then rows_per_wg * code_bytes rounded up to 16
    uint64_t row_blocks;     // ceil(n / rows_per_wg)
    unsigned gather_grid;    // min(row_blocks, kDecodeMaxGrid), at least 1
    // the rotation
    int reg, tile;           // register tile edge per lane; tile = kDecodeLanes * reg rows and columns per workgroup
    int col_tiles;           // ceil(dim / tile)
    uint64_t row_tiles;      // ceil(n / tile)
    uint64_t rot_grid;       // row_tiles * col_tiles workgroups, row-tile major
    size_t rot_lds;          // static LDS: 2 * kDecodeStage * tile floats, the window of y and the window of the rotation
    // the error pass
    uint64_t err_grid;       // ceil(n / kDecodeErrTile)
};

constexpr bool pq_decode_plan_shape_ok(int sq_count, int sq_bits) {
    return sq_bits == 4    ? (sq_count == 16 || sq_count == 32)
           : sq_bits == 8  ? (sq_count == 4 || sq_count == 8 || sq_count == 16)
           : sq_bits == 16 ? (sq_count == 2 || sq_count == 4 || sq_count == 8)
                           : false;
}

constexpr int pq_decode_max_dim(int sq_bits) { return sq_bits == 4 ? 2048 : 4096; }   // the encoders' limits

// One pass of n <= kDecodeChunk rows.  out_aligned16: the pass's first output float lies on a 16-byte boundary.  false: arguments
// the kernels do not take (the caller refuses them).  n == 0 plans no work (every grid 0 but gather_grid, which stays 1).
inline bool pq_decode_plan(int sq_count, int sq_bits, int dim, uint64_t n, bool out_aligned16, PqDecodePlan* p) {
    if (!pq_decode_plan_shape_ok(sq_count, sq_bits) || dim <= 0 || dim % sq_count != 0 || dim > pq_decode_max_dim(sq_bits)) return false;
    if (n > kDecodeChunk) return false;
    p->dim = dim;
    p->dsub = dim / sq_count;
    p->sq_count = sq_count;
    p->sq_bits = sq_bits;
    p->centroids = 1 << sq_bits;
    p->code_bytes = sq_bits == 4 ? sq_count / 2 : sq_bits == 8 ? sq_count : 2 * sq_count;
    p->vec = (dim % 4 == 0 && out_aligned16) ? 4 : 1;
    p->lanes_per_row = dim / p->vec;
    p->rows_per_wg = std::max(1, std::min(kDecodeMaxRows, kDecodeWG * kDecodeItems / p->lanes_per_row));
    p->cb_bytes = (size_t)p->centroids * (size_t)dim * sizeof(float);
    const size_t code_lds = ((size_t)p->rows_per_wg * (size_t)p->code_bytes + 15) / 16 * 16;
    p->cb_in_lds = sq_bits != 16 && p->cb_bytes + code_lds <= kDecodeLdsLimit;
    p->gather_lds = (p->cb_in_lds ? p->cb_bytes : 0) + code_lds;
    p->row_blocks = (n + (uint64_t)p->rows_per_wg - 1) / (uint64_t)p->rows_per_wg;
    p->gather_grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(p->row_blocks, kDecodeMaxGrid));
    p->reg = dim <= kDecodeLanes ? 1 : dim <= 2 * kDecodeLanes ? 2 : kDecodeMaxReg;
    p->tile = kDecodeLanes * p->reg;
    p->col_tiles = (dim + p->tile - 1) / p->tile;
    p->row_tiles = (n + (uint64_t)p->tile - 1) / (uint64_t)p->tile;
    p->rot_grid = p->row_tiles * (uint64_t)p->col_tiles;
    p->rot_lds = (size_t)2 * kDecodeStage * (size_t)p->tile * sizeof(float);
    p->err_grid = (n + kDecodeErrTile - 1) / kDecodeErrTile;
    return p->rot_grid < (1ull << 31) && p->gather_lds <= kDecodeLdsLimit && p->rot_lds <= 48 * 1024;
}

// The chain (i, c) that register (ra, rb) of lane `lane` of tile (ta, tb) owns — the rotation kernel's own indexing.  A row >= n or
// a column >= dim is outside the pass: the chain is not written.
constexpr uint64_t pq_decode_rot_row(int reg, uint64_t ta, int lane, int ra) { return (ta * kDecodeLanes + (uint64_t)(lane / kDecodeLanes)) * reg + ra; }
constexpr int pq_decode_rot_col(int reg, int tb, int lane, int rb) { return (tb * kDecodeLanes + lane % kDecodeLanes) * reg + rb; }

}  // namespace qadc
