// PQ decode: codes back to vectors.  Internal header shared by csrc/qadc_decode_kernel.hip,
// csrc/qadc_decode.cpp and the index forms in csrc/qadc_adc.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../host/pq_decode_plan.hpp"

namespace qadc {

// What one pass decodes, all in device memory.  rotation null: plain PQ.  K > 0: coarse [K][dim] is added, row i's centroid is
// assign[i].  assign (nullable with K == 0): a negative entry, or with K > 0 one >= K, makes row i a missing row — every float of
// its output 0x7FC00000.  codes [n][code bytes] in the encoder's layout, read byte by byte (no alignment); every code selects a
// centroid that exists (4 bits: a nibble, 8: a byte, 16: a word), so the gather stays inside the codebooks whatever the bytes are.
struct DecodeQuantizers {
    const float* codebooks;   // [sq_count][2^sq_bits][dsub], 16-byte aligned (the library's own allocation)
    const float* rotation;    // [dim][dim] or null
    const float* coarse;      // [K][dim] or null
    int K;
};

// out [n][dim] (4-byte aligned; 16-byte stores are used when the plan was made with out_aligned16), every float written.  n <=
// kDecodeChunk, n == 0 launches nothing.  hipErrorInvalidValue: a null pointer the pass needs.
hipError_t launch_pq_decode(const PqDecodePlan& p, const DecodeQuantizers& q, const int32_t* d_assign, const uint8_t* d_codes, uint64_t n,
                            float* d_out, hipStream_t stream);

// err[i] = the chain acc = fmaf(d, d, acc), d = vectors[i][c] - x[i][c], over ascending c from 0.0f; every err[i], i < n, written.
hipError_t launch_pq_decode_err(const float* d_vectors, const float* d_x, uint64_t n, int dim, float* d_err, hipStream_t stream);

namespace host {
// What every entry point runs once its inputs lie in device memory (csrc/qadc_decode.cpp): n rows in passes of kDecodeChunk, queued
// on `stream`, nothing waits.  d_vectors / d_err null: no error pass.  Returns a QADC_* code (QADC_E_ARG: a shape the plan refuses).
int decode_passes(int sq_count, int sq_bits, int dim, const DecodeQuantizers& q, const int32_t* d_assign, const uint8_t* d_codes, uint64_t n,
                  const float* d_vectors, float* d_out, float* d_err, hipStream_t stream);
// The shape checks of every decode entry point, before the first HIP call: the encoders' pairs and limits.
int decode_shape_check(int sq_count, int sq_bits, int dim);
}  // namespace host

// A partition as the lookup and the row gather of the index forms read it (the float-ADC engine's Part4, for owned indexes too).
struct DecodePart {
    const uint8_t* codes;
    const uint32_t* labels;   // null: keyed key_base + position
    uint32_t key_base;
    uint32_t size;
};

// Lookup, step 3: one pass over the index's keys.  A row whose key is marked in the bitmap (bit key - lo, inside [0, last]) finds
// its key among d_sorted [distinct] (ascending, distinct) and lowers d_slots[that index] to (partition << 32 | row) with a 64-bit
// atomicMin.  d_slots preset to ~0ull by the caller.  max_size: the largest partition.
hipError_t launch_reconstruct_find(const DecodePart* d_parts, int parts, uint32_t max_size, const uint32_t* d_bitmap, uint32_t lo, uint32_t last,
                                   const uint32_t* d_sorted, uint64_t distinct, unsigned long long* d_slots, hipStream_t stream);
// Lookup, step 4: d_where[i] = d_slots[index of d_keys[i] in d_sorted] for i < count.
hipError_t launch_reconstruct_read(const uint32_t* d_keys, uint64_t count, const uint32_t* d_sorted, uint64_t distinct,
                                   const unsigned long long* d_slots, unsigned long long* d_where, hipStream_t stream);
// The pass buffer of the index forms: for i < count, with w = d_where[i]: d_pass_assign[i] = -1 and a zero code row where w is
// ~0ull, else the partition and a copy of its row's code_bytes bytes (nibble, byte or word rows alike).
hipError_t launch_reconstruct_gather(const DecodePart* d_parts, const unsigned long long* d_where, uint64_t count, int code_bytes,
                                     int32_t* d_pass_assign, uint8_t* d_pass_codes, hipStream_t stream);
// d_where[i] = (part << 32) | (first + i) for i < count: rows by position (no lookup)
hipError_t launch_reconstruct_iota(uint32_t part, uint32_t first, uint64_t count, unsigned long long* d_where, hipStream_t stream);
// d_dst[i] = d_src[i] for i < count: a caller's device list into the library's own scratch (the caller's memory is read by kernels only)
hipError_t launch_decode_copy_u32(const uint32_t* d_src, uint64_t count, uint32_t* d_dst, hipStream_t stream);
// d_dst [count] uint64 at a 4-byte aligned address of the caller's: entry i written as its two little-endian 32-bit words
hipError_t launch_decode_copy_where(const unsigned long long* d_src, uint64_t count, uint32_t* d_dst, hipStream_t stream);

}  // namespace qadc
