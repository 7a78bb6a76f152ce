// PQ decode: codes back to vectors (include/qadc.h "Reconstruction").  Geometry: host/pq_decode_plan.hpp;
// CPU twin of every float: host/pq_decode.hpp.  Built with -ffp-contract=off; every fused operation is explicit.
//
//   pq_decode_gather_kernel   no rotation: a copy of codebook floats (plus one float add with a coarse quantizer), bounded by the
//                             bytes it writes.  A workgroup stages the code bytes of a block of rows through LDS (each read once,
//                             coalesced), then every lane owns VEC consecutive components of a row and stores them at once.
//   pq_decode_rotate_kernel   rotation: ONE chain acc = fmaf(y[r], rotation[r][c], acc) per (row, column) over ascending r.  A lane
//                             owns REG x REG whole chains; the workgroup stages windows of gathered y and of the rotation's rows
//                             through LDS (opq_cross_kernel's shape with the walk over r).  No split chain, no atomic, no MFMA.
//   pq_decode_err_kernel      ONE chain per row over ascending columns; the differences are staged through LDS so that the reads
//                             of both operands are coalesced.
//   reconstruct_*_kernel      the lookup of the index forms: key -> smallest (partition, row), then the rows' codes into a pass.
#include "qadc_decode.h"

namespace qadc {

namespace {

__device__ __forceinline__ uint32_t code_of(const uint8_t* row, int m, int sq_bits) {
    if (sq_bits == 4) return ((uint32_t)row[m >> 1] >> (4 * (m & 1))) & 15u;
    if (sq_bits == 8) return row[m];
    return (uint32_t)row[2 * m] | ((uint32_t)row[2 * m + 1] << 8);
}

__device__ __forceinline__ bool row_missing(const int32_t* assign, uint64_t i, int K, int32_t* a) {
    *a = assign ? assign[i] : 0;
    return assign && (*a < 0 || (K > 0 && *a >= K));
}

__device__ __forceinline__ float nan_fill() { return __uint_as_float(0x7FC00000u); }

// a NaN that arithmetic made or passed on is written as the canonical one (payloads differ between processors)
__device__ __forceinline__ float canonical(float v) { return v != v ? nan_fill() : v; }

template <int VEC, bool CB_LDS>
__global__ __launch_bounds__(kDecodeWG) void pq_decode_gather_kernel(DecodeQuantizers q, const int32_t* __restrict__ assign,
                                                                     const uint8_t* __restrict__ codes, uint64_t n, PqDecodePlan p,
                                                                     float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* cbs = reinterpret_cast<float*>(smem);
    uint8_t* cs = smem + (CB_LDS ? p.cb_bytes : 0);               // cb_bytes is a multiple of 64
    const int tid = threadIdx.x;
    if (CB_LDS) {
        const uint32_t quads = (uint32_t)(p.cb_bytes / 16);
        const float4* src = reinterpret_cast<const float4*>(q.codebooks);
        for (uint32_t e = tid; e < quads; e += kDecodeWG) reinterpret_cast<float4*>(cbs)[e] = src[e];
    }
    const float* cb = CB_LDS ? cbs : q.codebooks;
    for (uint64_t blk = blockIdx.x; blk < p.row_blocks; blk += gridDim.x) {
        const uint64_t row0 = blk * (uint64_t)p.rows_per_wg;
        const uint32_t rows = (uint32_t)min((uint64_t)p.rows_per_wg, n - row0);
        __syncthreads();                                          // the gather of the previous block is over
        const uint32_t nbytes = rows * (uint32_t)p.code_bytes;
        const uint8_t* src = codes + row0 * (uint64_t)p.code_bytes;
        for (uint32_t b = tid; b < nbytes; b += kDecodeWG) cs[b] = src[b];
        __syncthreads();                                          // (the first one also covers the staged codebooks)
        const uint32_t items = rows * (uint32_t)p.lanes_per_row;
        for (uint32_t e = tid; e < items; e += kDecodeWG) {
            const uint32_t r = e / (uint32_t)p.lanes_per_row;
            const int c = (int)(e - r * (uint32_t)p.lanes_per_row) * VEC;
            const uint64_t i = row0 + r;
            int32_t a;
            const bool missing = row_missing(assign, i, q.K, &a);
            float v[VEC];
            if (missing) {
#pragma unroll
                for (int k = 0; k < VEC; ++k) v[k] = nan_fill();
            } else {
                const uint8_t* row = cs + r * (uint32_t)p.code_bytes;
                if (VEC == 4 && (p.dsub & 3) == 0) {              // the four components lie in one centroid: one 16-byte read
                    const int m = c / p.dsub, d = c - m * p.dsub;
                    const float4 t = *reinterpret_cast<const float4*>(cb + ((size_t)m * p.centroids + code_of(row, m, p.sq_bits)) * p.dsub + d);
                    v[0] = t.x;
                    v[1 % VEC] = t.y;
                    v[2 % VEC] = t.z;
                    v[3 % VEC] = t.w;
                } else {
#pragma unroll
                    for (int k = 0; k < VEC; ++k) {
                        const int b = c + k, m = b / p.dsub, d = b - m * p.dsub;
                        v[k] = cb[((size_t)m * p.centroids + code_of(row, m, p.sq_bits)) * p.dsub + d];
                    }
                }
                if (q.K > 0) {
                    const float* cen = q.coarse + (size_t)a * p.dim + c;
#pragma unroll
                    for (int k = 0; k < VEC; ++k) v[k] = canonical(v[k] + cen[k]);
                }
            }
            float* dst = out + i * (uint64_t)p.dim + (uint64_t)c;
            if (VEC == 4)
                *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1 % VEC], v[2 % VEC], v[3 % VEC]);
            else
                dst[0] = v[0];
        }
    }
}

template <int REG>
__global__ __launch_bounds__(kDecodeWG) void pq_decode_rotate_kernel(DecodeQuantizers q, const int32_t* __restrict__ assign,
                                                                     const uint8_t* __restrict__ codes, uint64_t n, PqDecodePlan p,
                                                                     float* __restrict__ out) {
    constexpr int TILE = kDecodeLanes * REG;
    constexpr int kStageRegs = kDecodeStage * TILE / kDecodeWG;   // staged entries per lane and window: 2, 4 or 8
    __shared__ __attribute__((aligned(16))) float ys[kDecodeStage][TILE];
    __shared__ __attribute__((aligned(16))) float rs[kDecodeStage][TILE];
    const int tid = threadIdx.x;
    const uint32_t ta = blockIdx.x / (uint32_t)p.col_tiles;
    const int tb = (int)(blockIdx.x - ta * (uint32_t)p.col_tiles);
    const uint64_t i0 = (uint64_t)ta * TILE;
    const int c0 = tb * TILE;
    const int la = tid / kDecodeLanes, lb = tid % kDecodeLanes;

    float acc[REG][REG];
#pragma unroll
    for (int ra = 0; ra < REG; ++ra)
#pragma unroll
        for (int rb = 0; rb < REG; ++rb) acc[ra][rb] = 0.0f;

    for (int r0 = 0; r0 < p.dim; r0 += kDecodeStage) {
        const int steps = min(kDecodeStage, p.dim - r0);
        __syncthreads();                                          // the walk over the previous window is over
#pragma unroll
        for (int k = 0; k < kStageRegs; ++k) {
            const int e = tid + kDecodeWG * k;
            {                                                     // the rotation's rows r0 .. r0 + steps, columns of the tile: coalesced
                const int s = e / TILE, c = e - s * TILE, col = c0 + c;
                rs[s][c] = (s < steps && col < p.dim) ? q.rotation[(size_t)(r0 + s) * p.dim + col] : 0.0f;
            }
            {                                                     // y gathered while staging: four consecutive r per row side by side
                const int s = (e & 3) + 4 * (e / (4 * TILE)), a = (e >> 2) % TILE;
                const uint64_t i = i0 + (uint64_t)a;
                float yv = 0.0f;
                if (s < steps && i < n) {
                    const int b = r0 + s, m = b / p.dsub, d = b - m * p.dsub;
                    const uint32_t code = code_of(codes + i * (uint64_t)p.code_bytes, m, p.sq_bits);
                    yv = q.codebooks[((size_t)m * p.centroids + code) * p.dsub + d];
                }
                ys[s][a] = yv;
            }
        }
        __syncthreads();
        for (int s = 0; s < steps; ++s) {                         // ascending r: the pinned order
            float yr[REG], rr[REG];
#pragma unroll
            for (int r = 0; r < REG; ++r) {
                yr[r] = ys[s][la * REG + r];
                rr[r] = rs[s][lb * REG + r];
            }
#pragma unroll
            for (int ra = 0; ra < REG; ++ra)
#pragma unroll
                for (int rb = 0; rb < REG; ++rb) acc[ra][rb] = __fmaf_rn(yr[ra], rr[rb], acc[ra][rb]);
        }
    }
#pragma unroll
    for (int ra = 0; ra < REG; ++ra) {
        const uint64_t i = pq_decode_rot_row(REG, ta, tid, ra);
        if (i >= n) continue;
        int32_t a;
        const bool missing = row_missing(assign, i, q.K, &a);
#pragma unroll
        for (int rb = 0; rb < REG; ++rb) {
            const int c = pq_decode_rot_col(REG, tb, tid, rb);
            if (c >= p.dim) continue;
            float v = acc[ra][rb];
            if (!missing && q.K > 0) v = v + q.coarse[(size_t)a * p.dim + c];
            out[i * (uint64_t)p.dim + (uint64_t)c] = missing ? nan_fill() : canonical(v);
        }
    }
}

__global__ __launch_bounds__(kDecodeWG) void pq_decode_err_kernel(const float* __restrict__ vectors, const float* __restrict__ x, uint64_t n,
                                                                  int dim, float* __restrict__ err) {
    __shared__ float ds[kDecodeErrTile][kDecodeErrTile + 1];      // + 1: a lane walks its row without a bank conflict
    const int tid = threadIdx.x;
    const uint64_t i0 = (uint64_t)blockIdx.x * kDecodeErrTile;
    float acc = 0.0f;
    for (int c0 = 0; c0 < dim; c0 += kDecodeErrTile) {
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kDecodeErrTile * kDecodeErrTile / kDecodeWG; ++k) {
            const int e = tid + kDecodeWG * k, r = e / kDecodeErrTile, c = e % kDecodeErrTile, col = c0 + c;
            const uint64_t i = i0 + (uint64_t)r;
            float d = 0.0f;
            if (i < n && col < dim) d = vectors[i * (uint64_t)dim + col] - x[i * (uint64_t)dim + col];
            ds[r][c] = d;
        }
        __syncthreads();
        if (tid < kDecodeErrTile) {
            const int cols = min(kDecodeErrTile, dim - c0);
            for (int c = 0; c < cols; ++c) {                      // ascending column: the pinned order
                const float d = ds[tid][c];
                acc = __fmaf_rn(d, d, acc);
            }
        }
    }
    if (tid < kDecodeErrTile && i0 + (uint64_t)tid < n) err[i0 + (uint64_t)tid] = canonical(acc);
}

// ---- the lookup of the index forms ----

// index of `key` in sorted [distinct] (ascending, distinct); the caller knows it is there
__device__ __forceinline__ uint64_t slot_of(const uint32_t* __restrict__ sorted, uint64_t distinct, uint32_t key) {
    uint64_t lo = 0, hi = distinct;                               // the first entry >= key lies in [lo, hi)
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (sorted[mid] <= key) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kDecodeWG) void reconstruct_find_kernel(const DecodePart* __restrict__ parts, const uint32_t* __restrict__ bitmap,
                                                                     uint32_t lo, uint32_t last, const uint32_t* __restrict__ sorted,
                                                                     uint64_t distinct, unsigned long long* __restrict__ slots) {
    const DecodePart pt = parts[blockIdx.y];
    for (uint64_t r = (uint64_t)blockIdx.x * kDecodeWG + threadIdx.x; r < pt.size; r += (uint64_t)gridDim.x * kDecodeWG) {
        const uint32_t key = pt.labels ? pt.labels[r] : pt.key_base + (uint32_t)r;
        const uint32_t bit = key - lo;                            // modulo 2^32: a key below lo lands above last
        if (bit > last || !((bitmap[bit >> 5] >> (bit & 31)) & 1u)) continue;
        atomicMin(&slots[slot_of(sorted, distinct, key)], ((unsigned long long)blockIdx.y << 32) | (unsigned long long)r);
    }
}

__global__ __launch_bounds__(kDecodeWG) void reconstruct_read_kernel(const uint32_t* __restrict__ keys, uint64_t count,
                                                                     const uint32_t* __restrict__ sorted, uint64_t distinct,
                                                                     const unsigned long long* __restrict__ slots,
                                                                     unsigned long long* __restrict__ where) {
    const uint64_t i = (uint64_t)blockIdx.x * kDecodeWG + threadIdx.x;
    if (i < count) where[i] = slots[slot_of(sorted, distinct, keys[i])];
}

__global__ __launch_bounds__(kDecodeWG) void reconstruct_gather_kernel(const DecodePart* __restrict__ parts,
                                                                       const unsigned long long* __restrict__ where, uint64_t count,
                                                                       int code_bytes, int32_t* __restrict__ pass_assign,
                                                                       uint8_t* __restrict__ pass_codes) {
    const uint64_t e = (uint64_t)blockIdx.x * kDecodeWG + threadIdx.x;   // one lane per (row, code byte)
    const uint64_t i = e / (uint64_t)code_bytes;
    if (i >= count) return;
    const int b = (int)(e - i * (uint64_t)code_bytes);
    const unsigned long long w = where[i];
    const bool missing = w == ~0ull;
    if (b == 0) pass_assign[i] = missing ? -1 : (int32_t)(w >> 32);
    pass_codes[e] = missing ? (uint8_t)0 : parts[w >> 32].codes[(w & 0xffffffffull) * (uint64_t)code_bytes + (uint64_t)b];
}

__global__ __launch_bounds__(kDecodeWG) void reconstruct_iota_kernel(uint32_t part, uint32_t first, uint64_t count,
                                                                     unsigned long long* __restrict__ where) {
    const uint64_t i = (uint64_t)blockIdx.x * kDecodeWG + threadIdx.x;
    if (i < count) where[i] = ((unsigned long long)part << 32) | ((unsigned long long)first + i);
}

template <typename T>
__global__ __launch_bounds__(kDecodeWG) void decode_copy_kernel(const T* __restrict__ src, uint64_t count, T* __restrict__ dst) {
    const uint64_t i = (uint64_t)blockIdx.x * kDecodeWG + threadIdx.x;
    if (i < count) dst[i] = src[i];
}

// a caller's where_out is 4-byte aligned: each entry goes out as its two little-endian words
__global__ __launch_bounds__(kDecodeWG) void decode_copy_where_kernel(const unsigned long long* __restrict__ src, uint64_t count,
                                                                      uint32_t* __restrict__ dst) {
    const uint64_t i = (uint64_t)blockIdx.x * kDecodeWG + threadIdx.x;
    if (i >= count) return;
    const unsigned long long w = src[i];
    dst[2 * i] = (uint32_t)w;
    dst[2 * i + 1] = (uint32_t)(w >> 32);
}

unsigned blocks_for(uint64_t items) { return (unsigned)((items + kDecodeWG - 1) / kDecodeWG); }

}  // namespace

hipError_t launch_pq_decode(const PqDecodePlan& p, const DecodeQuantizers& q, const int32_t* d_assign, const uint8_t* d_codes, uint64_t n,
                            float* d_out, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (n > kDecodeChunk || !q.codebooks || !d_codes || !d_out || (q.K > 0 && (!q.coarse || !d_assign))) return hipErrorInvalidValue;
    const dim3 wg(kDecodeWG);
    if (q.rotation) {
        const dim3 grid((unsigned)p.rot_grid);
        if (p.reg == 1)
            hipLaunchKernelGGL(pq_decode_rotate_kernel<1>, grid, wg, 0, stream, q, d_assign, d_codes, n, p, d_out);
        else if (p.reg == 2)
            hipLaunchKernelGGL(pq_decode_rotate_kernel<2>, grid, wg, 0, stream, q, d_assign, d_codes, n, p, d_out);
        else
            hipLaunchKernelGGL(pq_decode_rotate_kernel<4>, grid, wg, 0, stream, q, d_assign, d_codes, n, p, d_out);
        return hipGetLastError();
    }
    if (p.vec == 4 && (reinterpret_cast<uintptr_t>(d_out) & 15)) return hipErrorInvalidValue;
    const dim3 grid(p.gather_grid);
    if (p.vec == 4 && p.cb_in_lds)
        hipLaunchKernelGGL((pq_decode_gather_kernel<4, true>), grid, wg, p.gather_lds, stream, q, d_assign, d_codes, n, p, d_out);
    else if (p.vec == 4)
        hipLaunchKernelGGL((pq_decode_gather_kernel<4, false>), grid, wg, p.gather_lds, stream, q, d_assign, d_codes, n, p, d_out);
    else if (p.cb_in_lds)
        hipLaunchKernelGGL((pq_decode_gather_kernel<1, true>), grid, wg, p.gather_lds, stream, q, d_assign, d_codes, n, p, d_out);
    else
        hipLaunchKernelGGL((pq_decode_gather_kernel<1, false>), grid, wg, p.gather_lds, stream, q, d_assign, d_codes, n, p, d_out);
    return hipGetLastError();
}

hipError_t launch_pq_decode_err(const float* d_vectors, const float* d_x, uint64_t n, int dim, float* d_err, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (!d_vectors || !d_x || !d_err || dim <= 0 || n > kDecodeChunk) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pq_decode_err_kernel, dim3((unsigned)((n + kDecodeErrTile - 1) / kDecodeErrTile)), dim3(kDecodeWG), 0, stream, d_vectors,
                       d_x, n, dim, d_err);
    return hipGetLastError();
}

hipError_t launch_reconstruct_find(const DecodePart* d_parts, int parts, uint32_t max_size, const uint32_t* d_bitmap, uint32_t lo, uint32_t last,
                                   const uint32_t* d_sorted, uint64_t distinct, unsigned long long* d_slots, hipStream_t stream) {
    if (parts <= 0 || max_size == 0 || distinct == 0) return hipSuccess;
    if (parts > 65535) return hipErrorInvalidValue;
    const unsigned gx = std::min(blocks_for(max_size), 4096u);
    hipLaunchKernelGGL(reconstruct_find_kernel, dim3(gx, (unsigned)parts), dim3(kDecodeWG), 0, stream, d_parts, d_bitmap, lo, last, d_sorted,
                       distinct, d_slots);
    return hipGetLastError();
}

hipError_t launch_reconstruct_read(const uint32_t* d_keys, uint64_t count, const uint32_t* d_sorted, uint64_t distinct,
                                   const unsigned long long* d_slots, unsigned long long* d_where, hipStream_t stream) {
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(reconstruct_read_kernel, dim3(blocks_for(count)), dim3(kDecodeWG), 0, stream, d_keys, count, d_sorted, distinct, d_slots,
                       d_where);
    return hipGetLastError();
}

hipError_t launch_reconstruct_gather(const DecodePart* d_parts, const unsigned long long* d_where, uint64_t count, int code_bytes,
                                     int32_t* d_pass_assign, uint8_t* d_pass_codes, hipStream_t stream) {
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(reconstruct_gather_kernel, dim3(blocks_for(count * (uint64_t)code_bytes)), dim3(kDecodeWG), 0, stream, d_parts, d_where,
                       count, code_bytes, d_pass_assign, d_pass_codes);
    return hipGetLastError();
}

hipError_t launch_reconstruct_iota(uint32_t part, uint32_t first, uint64_t count, unsigned long long* d_where, hipStream_t stream) {
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(reconstruct_iota_kernel, dim3(blocks_for(count)), dim3(kDecodeWG), 0, stream, part, first, count, d_where);
    return hipGetLastError();
}

hipError_t launch_decode_copy_u32(const uint32_t* d_src, uint64_t count, uint32_t* d_dst, hipStream_t stream) {
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(decode_copy_kernel<uint32_t>, dim3(blocks_for(count)), dim3(kDecodeWG), 0, stream, d_src, count, d_dst);
    return hipGetLastError();
}

hipError_t launch_decode_copy_where(const unsigned long long* d_src, uint64_t count, uint32_t* d_dst, hipStream_t stream) {
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(decode_copy_where_kernel, dim3(blocks_for(count)), dim3(kDecodeWG), 0, stream, d_src, count, d_dst);
    return hipGetLastError();
}

}  // namespace qadc
