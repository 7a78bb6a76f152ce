// MI355X (gfx950 / CDNA4) kernels of the Quick-ADC scan engine.
//
// Replaces, on device, the reference's hot loop scan_avx_4<M> (simd_scan.hpp:125-187) and the
// float pre-scan scan_4<M> (query_common.hpp:59-90).  Nothing here is a translation of the AVX2
// code: the pshufb register lookup becomes an LDS gather against pair-fused, bank-replicated byte
// tables, the 16-code block transpose (simd_layout.hpp) is dropped in favour of plain row-major
// codes read with one coalesced 16-byte load per lane, and the sequential heap is replaced by a
// prefix-bound filter whose output is replayed on the host.
//
// The op is a gather + byte add bound by HBM reads: no MFMA.
#include "qadc_kernels.h"
#include "qadc_float_sum.h"
#include "qadc_front_nonfinite.h"
#include <cstdio>
#include <cstdlib>

#include <algorithm>
#include <atomic>
#include <cfloat>
#include <type_traits>

namespace qadc {

constexpr int kWG = 1024;       // threads per workgroup of the int8 scan (16 waves)

extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

// Dynamic-LDS opt-in above the default limit is a property of (kernel, DEVICE): it is requested once per device
// the kernel is launched on (an index on GPU 1 after one on GPU 0 in the same process needs its own opt-in), and a
// failure is kept for the host (take_launch_error) instead of being dropped.
static thread_local hipError_t g_launch_err = hipSuccess;

hipError_t take_launch_error() {
    const hipError_t e = g_launch_err;
    g_launch_err = hipSuccess;
    return e;
}

static void ensure_dynamic_lds(const void* fn, int bytes, std::atomic<uint64_t>& done_devices) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 63;
    const uint64_t bit = 1ull << dev;
    if (done_devices.load(std::memory_order_acquire) & bit) return;
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) { g_launch_err = e; return; }
    if (dev != 63) done_devices.fetch_or(bit, std::memory_order_release);
}

// ---------------------------------------------------------------------------------------------
// int8 scan
//
// LDS image (per workgroup): for byte position b of a code (b = 4g + j) the pair table
//     P_b[x] = T[2b][x & 15] + T[2b+1][x >> 4]          (<= 254, one byte)
// is stored at   region(g) + x*256 + (g&1)*128 + bank*4 + j     for bank = 0..31,
// region(g) = (g>>1) * 64 KiB.  A lane reads with bank = lane & 31, so the 32 lanes of a
// ds_read lane group hit 32 different banks whatever their x: conflict-free by construction.
// One dword holds the four tables of a group, so the 32-fold replication costs 64 KiB per
// 8 code bytes (M=16: 64 KiB, M=32: 128 KiB).
// The byte address x*256 + bank*4 is formed by ONE v_perm_b32 from the code dword and the
// lane constant; (g&1)*128 + j rides in the ds_read immediate offset.
// ---------------------------------------------------------------------------------------------
// 6- and 5-plane split forms: the code byte whose pair table sits in slot s of the LDS image when PLANES of the bytes 0..6
// are streamed and the others are deferred (6: j1; 5: j1 < j2):
// slots 0..PLANES-1 = the streamed bytes, in order; then the deferred ones, in order; slot 7 = byte 7.
template <int PLANES>
__host__ __device__ __forceinline__ uint32_t split_byte(uint32_t s, uint32_t j1, uint32_t j2 = 7u) {
    if (PLANES == 6) return s < 6u ? s + (s >= j1 ? 1u : 0u) : (s == 6u ? j1 : 7u);
    if (s < 5u) {
        const uint32_t b = s + (s >= j1 ? 1u : 0u);
        return b + (b >= j2 ? 1u : 0u);
    }
    return s == 5u ? j1 : (s == 6u ? j2 : 7u);
}

template <int M>
struct ScanCfg {
    static constexpr int CS = M / 2;             // code bytes
    static constexpr int DW = M / 8;             // dwords per code
    static constexpr int CPL = 16 / CS;          // codes per 16-byte lane load
    static constexpr int TABLE_BYTES = (M / 16) * 65536;
    static constexpr int STAGE_OFF = TABLE_BYTES;          // int8 [M][16] staging copy
    static constexpr int HIST_OFF = STAGE_OFF + M * 16;    // u32 [128] prefix histogram
    static constexpr int BOUND_OFF = HIST_OFF + 512;       // u32 bound
    static constexpr int LDS_BYTES = BOUND_OFF + 16;
};

// PERM = 6 or 5 (those split forms): slot s of the image holds the pair table of code byte split_byte<PERM>(s, defer, defer2)
// instead of byte s.
template <int M, int PERM = 0>
__device__ __forceinline__ void build_pair_tables(const int8_t* __restrict__ qt, uint32_t defer = 0, uint32_t defer2 = 7) {
    using C = ScanCfg<M>;
    const int t = threadIdx.x;
    // stage the int8 table (M*16 bytes) into LDS
    if (t < M * 4) reinterpret_cast<uint32_t*>(smem + C::STAGE_OFF)[t] = reinterpret_cast<const uint32_t*>(qt)[t];
    __syncthreads();
    const unsigned char* T = smem + C::STAGE_OFF;
    // The image is written in ADDRESS order: thread t stores the 16-byte units t, t + kWG, ...; a wave's ds_write_b128 covers
    // 1 KiB contiguous — every bank once.  (Until round 4 a thread wrote the 128-byte row of one (dword g, byte x) pair by
    // itself: the rows of a wave's lanes lie 256 bytes apart, i.e. in the SAME banks — a 32-way conflict on every store,
    // ~4 K LDS cycles per 64 KiB image instead of ~256.)  A wave's units of iteration k belong to 8 (g, x) pairs, 8 lanes each;
    // lane l computes pair l's dword once and ds_bpermute hands it to the lanes that replicate it.
    constexpr int kIter = C::TABLE_BYTES / 16 / kWG;     // 16x4: 4, 32x4: 8 units per thread
    const uint32_t lane = (uint32_t)t & 63u, wave = (uint32_t)t >> 6;
    uint32_t w = 0;
    {
        const uint32_t pi = lane & (8u * kIter - 1u);    // (16x4: lanes 32..63 repeat 0..31)
        const uint32_t k = pi >> 3, within = pi & 7u;
        const uint32_t x = (k & 3u) * 64u + wave * 4u + (within >> 1);
        const uint32_t g = (k >> 2) * 2u + (within & 1u);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t b = PERM ? split_byte<PERM ? PERM : 6>(4u * g + j, defer, defer2) : 4u * g + j;
            const uint32_t v = (uint32_t)T[(2 * b) * 16 + (x & 15u)] + (uint32_t)T[(2 * b + 1) * 16 + (x >> 4)];
            w |= v << (8 * j);
        }
    }
#pragma unroll
    for (int k = 0; k < kIter; ++k) {
        const uint32_t wk = (uint32_t)__builtin_amdgcn_ds_bpermute((int)((k * 8u + (lane >> 3)) * 4u), (int)w);
        *reinterpret_cast<uint4*>(smem + ((size_t)k * kWG + t) * 16) = make_uint4(wk, wk, wk, wk);
    }
}

// inclusive wave scan on the DPP path (row shifts + row broadcasts, 7 VALU operations) — __shfl_up goes through the LDS
// crossbar, ~100 cycles per hop in a dependent chain of six
__device__ __forceinline__ uint32_t dpp_wave_incl_sum(uint32_t x) {
    uint32_t v = x;
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xf, 0xf, false);   // row_shr:1
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xf, 0xf, false);   // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x113, 0xf, 0xf, false);   // row_shr:3
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xe, false);   // row_shr:4, banks 1-3
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xc, false);   // row_shr:8, banks 2-3
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);   // row_bcast:15 -> rows 1, 3
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);   // row_bcast:31 -> rows 2, 3
    return v;
}

// bound = smallest v with #(emitted candidates of all earlier levels with value <= v) >= R, else 127.
// Valid for every code of this level because those candidates all precede it in scan order.
__device__ __forceinline__ uint32_t prefix_bound(const QueryState* qs, int level, uint32_t R, uint32_t* lds_hist,
                                                 uint32_t* lds_bound) {
    const int t = threadIdx.x;
    if (t < 128) {
        uint32_t c = 0;
        for (int l = 0; l < level; ++l) c += qs->hist[l * 128 + t];
        lds_hist[t] = c;
    }
    __syncthreads();
    if (t < 64) {
        const uint32_t c0 = lds_hist[2 * t], c1 = lds_hist[2 * t + 1];
        const uint32_t incl = dpp_wave_incl_sum(c0 + c1);
        const uint32_t excl = incl - (c0 + c1);
        const uint64_t reached = __builtin_amdgcn_ballot_w64(incl >= R);
        uint32_t b = excl + c0 >= R ? 2 * t : 2 * t + 1;         // (meaningful in the first lane that reaches R)
        b = reached ? min((uint32_t)__builtin_amdgcn_readlane((int)b, (int)__builtin_ctzll(reached ? reached : 1)), 127u) : 127u;
        if (t == 0) *lds_bound = b;
    }
    __syncthreads();
    return *lds_bound;
}

__device__ __noinline__ void emit_candidate(QueryState* qs, CandHeader* hdr, Cand* __restrict__ region, uint32_t cap,
                                            const uint32_t* __restrict__ labels, uint32_t key_base, uint32_t order,
                                            uint32_t dup_pos, uint32_t dup_reps, uint32_t pos, uint32_t val) {
    const uint32_t reps = pos == dup_pos ? dup_reps : 0u;
    const uint32_t slot = atomicAdd(&qs->count, 1u);
    if (slot < cap) {
        Cand c;
        c.order = order | (reps << 20);
        c.pos = pos;
        c.key = labels ? labels[pos] : key_base + pos;
        c.val = val;
        region[slot] = c;
    } else {
        atomicAdd(&hdr->overflow, 1u);
    }
    if (reps) atomicAdd(&qs->reps, reps);
    atomicAdd(&qs->hist[(order >> 16) * 128 + val], 1u);
}

// The pair tables start at LDS address 0 (these kernels have no static __shared__, so the dynamic
// region begins there — checked once per workgroup by lds_base_is_zero()); the lookups therefore use
// ABSOLUTE LDS addresses, which spares one "add the array base" VALU instruction per lookup.
typedef const __attribute__((address_space(3))) unsigned char* lds_bytes_t;

__device__ __forceinline__ void lds_base_is_zero() {
    if (reinterpret_cast<uintptr_t>((lds_bytes_t)smem) != 0) __builtin_trap();
}

template <int M>
__device__ __forceinline__ uint32_t pair_sum(const uint32_t* d, uint32_t lane_lo, uint32_t lane_hi) {
    uint32_t s = 0;
#pragma unroll
    for (int w = 0; w < M / 8; ++w) {
        const uint32_t lo = (w >> 1) ? lane_hi : lane_lo;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            // byte0 = bank*4, byte1 = code byte k, byte2 = region bit, byte3 = 0
            const uint32_t a = __builtin_amdgcn_perm(d[w], lo, 0x0c020000u | ((4u + k) << 8));
            s += *reinterpret_cast<lds_bytes_t>(static_cast<uintptr_t>(a + (w & 1) * 128 + k));
        }
    }
    return s;
}

// Compile-time forms: NT = non-temporal loads, CHUNK = each workgroup owns a contiguous run of tiles instead of a grid-stride,
// PROBE = replace the LDS lookups by a trivial reduction (the streaming-ceiling diagnostic of bench.py; results meaningless).
// U = 2 16-KiB tiles in flight per lane (1 and 4, and a software-prefetch form, were measured in rounds 1-2: profiles/README.md).
template <int M, bool NT, bool CHUNK, bool PROBE>
__global__ __launch_bounds__(kWG, (M == 16 ? 8 : 4)) void scan_i8_kernel(
    const ScanItem* __restrict__ items, const int8_t* __restrict__ qtables, QueryState* __restrict__ qstates,
    CandHeader* __restrict__ hdr, Cand* __restrict__ out, uint32_t cand_cap, uint32_t R, uint32_t sib_items) {
    using C = ScanCfg<M>;
    constexpr int U = 2;
    // Workgroup -> (run, position in the run).  2-D launch: blockIdx.y = run.  Sibling-major 1-D launch
    // (sib_items = runs in the launch, all over the SAME code range, one per query): the hardware deals consecutive
    // workgroup ids round-robin to the 8 XCDs, so ids that are equal mod 8 share an L2; the decode below puts the
    // sib_items workgroups that read the same tiles (one per query) on one XCD, dispatched back to back: the first
    // of them pulls a tile from HBM, the others find it in that XCD's L2.
    uint32_t bx = blockIdx.x, by = blockIdx.y, G = gridDim.x;
    if (sib_items) {
        G = gridDim.x / sib_items;
        if ((G & 7u) == 0) {
            const uint32_t r = blockIdx.x >> 3;
            by = r % sib_items;
            bx = (r / sib_items) * 8u + (blockIdx.x & 7u);
        } else {
            by = blockIdx.x % sib_items;
            bx = blockIdx.x / sib_items;
        }
    }
    const ScanItem it = items[by];
    QueryState* qs = qstates + it.query;
    out += (uint64_t)it.query * cand_cap;                       // this query's candidate region

    build_pair_tables<M>(qtables + (uint64_t)it.table * (M * 16));
    const uint32_t bound = prefix_bound(qs, it.order >> 16, R, reinterpret_cast<uint32_t*>(smem + C::HIST_OFF),
                                        reinterpret_cast<uint32_t*>(smem + C::BOUND_OFF));

    const uint32_t tid = threadIdx.x;
    const uint32_t lane_lo = (tid & 31u) * 4u;
    const uint32_t lane_hi = lane_lo | 0x10000u;
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    // codes live in global memory: say so, or the non-temporal builtin falls back to FLAT loads
    typedef const __attribute__((address_space(1))) u32x4* gvec_t;
    const gvec_t src = (gvec_t)(uintptr_t)it.codes;
    lds_base_is_zero();
    const uint32_t n = it.n;
    const uint32_t nvec = (n + C::CPL - 1) / C::CPL;            // 16-byte vectors in the run
    const uint32_t ntiles = (nvec + kWG - 1) / kWG;
    // tile sequence of this workgroup: first, first+step, ... < last
    uint32_t first = bx, last = ntiles, step = G;
    if (CHUNK) {
        const uint32_t per = (ntiles + G - 1) / G;
        first = bx * per;
        last = min(ntiles, first + per);
        step = 1;
    }

    // FULL = every lane of every tile of the iteration holds CPL valid codes: no predicates, no branches
    // around the lookups, so the compiler can keep all U*CPL*CS ds_reads of an iteration in flight.
    auto load_tiles = [&](uint32_t t0, u32x4 (&v)[U], uint32_t (&e)[U], auto full) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t t = t0 + u * step;
            e[u] = t * kWG + tid;                               // vector index
            if (decltype(full)::value) {
                v[u] = NT ? __builtin_nontemporal_load(src + e[u]) : src[e[u]];
            } else {
                v[u] = u32x4{0, 0, 0, 0};
                if (t < last && e[u] < nvec) v[u] = NT ? __builtin_nontemporal_load(src + e[u]) : src[e[u]];
                else e[u] = 0xffffffffu;
            }
        }
    };
    auto process = [&](const u32x4 (&v)[U], const uint32_t (&e)[U], auto full) {
        uint32_t cand[U * C::CPL];
        uint32_t best = 127u;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t d[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
            for (int c = 0; c < C::CPL; ++c) {
                uint32_t s;
                if (PROBE) {
                    s = 0;
#pragma unroll
                    for (int w = 0; w < C::DW; ++w) s ^= d[c * C::DW + w];
                    s = (s == 0x12345678u) ? 0u : 200u;
                } else {
                    s = pair_sum<M>(d + c * C::DW, lane_lo, lane_hi);
                }
                uint32_t cv = min(s, 127u);
                if (!decltype(full)::value) {
                    // lanes past the end of the run never qualify: 127 is not < bound (bound <= 127)
                    const bool live = e[u] != 0xffffffffu && e[u] * C::CPL + c < n;
                    cv = live ? cv : 127u;
                }
                cand[u * C::CPL + c] = cv;
                best = min(best, cv);
            }
        }
        if (__builtin_expect(best < bound, 0)) {                // rare: one branch per U tiles
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int c = 0; c < C::CPL; ++c)
                    if (cand[u * C::CPL + c] < bound)
                        emit_candidate(qs, hdr, out, cand_cap, it.labels, it.key_base, it.order, it.dup_pos, it.dup_reps,
                                       it.pos0 + e[u] * C::CPL + c, cand[u * C::CPL + c]);
        }
    };
    using full_t = std::integral_constant<bool, true>;
    using part_t = std::integral_constant<bool, false>;
    // tiles [0, tiles_full) contain only complete vectors of complete codes
    const uint32_t tiles_full = (n / C::CPL) / kWG;
    const uint32_t full_last = min(last, tiles_full);

    uint32_t t0 = first;
    for (; t0 + (U - 1) * step < full_last; t0 += step * U) {       // steady state: unpredicated
        u32x4 v[U];
        uint32_t e[U];
        load_tiles(t0, v, e, full_t());
        process(v, e, full_t());
    }
    for (; t0 < last; t0 += step * U) {                              // ragged end of the run
        u32x4 v[U];
        uint32_t e[U];
        load_tiles(t0, v, e, part_t());
        process(v, e, part_t());
    }
}

// ---------------------------------------------------------------------------------------------
// Split form of scan_i8_kernel (16x4, one query per pass): the run is streamed from the partition's byte-plane copy of
// code bytes 0-6 (kSplitTile, launch_split_copy), PLANES = 7, 6 or 5 of the 8 bytes per code.  Pair-table entries are >= 0, so
// the sum over any subset of the bytes is a lower bound on the code's value: a code with min(127, partial) >= bound cannot
// be a candidate and is dropped without its deferred bytes.  A survivor (partial < bound) reads them from the row-major
// array and is finished exactly as in scan_i8_kernel: cand = min(127, partial + the deferred pair entries), emitted when
// cand < bound.  Survivors are resolved one iteration late: their row-major loads are issued behind the NEXT iteration's
// plane loads, so the dependent misses overlap the stream instead of stalling it.  A lane holds 16 codes per iteration (one
// 16-byte load per plane: a wave reads 1 KiB contiguous of each plane, a workgroup one tile = PLANES x 16 KiB).
//   PLANES = 7: planes 0-6, byte 7 deferred.
//   PLANES = 6: the query's table also defers byte plane_sel[table] (0..6, plane_choice below: the byte whose pair entries
//     are smallest, i.e. the one that tightens the partial sum least) and skips that plane of every tile.  The LDS image is
//     built permuted (split6_byte: streamed bytes in slots 0-5, the deferred two in slots 6 and 7) and the permutation is
//     folded into the six uniform plane offsets, so the loop's lookups are those of PLANES = 7 without its last.  Survivors
//     are some 20 times as frequent as with 7 planes, so they are resolved by a loop over the lane's set
//     survivor bits (the wave runs as many trips as its busiest lane has survivors, usually one), not by a sweep of 16 slots.
//   PLANES = 5: the table defers two bytes j1 < j2 of 0..6 (plane_choice5: the two that tighten the partial sum least beyond
//     their minima) and byte 7; plane_sel holds 2 bytes per table here: j1 | j2 << 4, and the slack c = min(127, the sum of
//     the three deferred pair tables' minima).  Every code's full sum is >= partial + c, so a code whose 5-byte partial is not
//     below bound - c cannot be a candidate: the survivor test is min(127, partial) < bsurv = max(bound - c, 0) (0: no code
//     survives), which brings the survivor rate of 5 planes down to that of the 6-plane form without slack.
//     A survivor is finished with all three deferred entries and emitted against the real bound.  The 6- and 7-plane forms
//     keep their test (bound itself).
// PROBE: XOR of the streamed planes, no deferred bytes (the streaming ceiling of this form; results meaningless).
// surv (profile option only, else null): counts the survivors of the 6- or 5-plane form, one atomicAdd per workgroup at exit (one
// per wave, half a million to one address per launch, cost the headline 3 ms a step; the 7-plane form has no register left
// for the count and does not report it).
// ---------------------------------------------------------------------------------------------
template <int PLANES, bool NT, bool CHUNK, bool PROBE>
__global__ __launch_bounds__(kWG, 8) void scan_i8_split_kernel(
    const ScanItem* __restrict__ items, const int8_t* __restrict__ qtables, QueryState* __restrict__ qstates,
    CandHeader* __restrict__ hdr, Cand* __restrict__ out, uint32_t cand_cap, uint32_t R,
    const uint8_t* __restrict__ plane_sel, unsigned long long* __restrict__ surv) {
    static_assert(PLANES >= 5 && PLANES <= (int)kSplitBytes, "5, 6 or all 7 planes of the copy");
    using C = ScanCfg<16>;
    const ScanItem it = items[blockIdx.y];
    QueryState* qs = qstates + it.query;
    out += (uint64_t)it.query * cand_cap;
    uint32_t defer = 6;                                         // PLANES == 6: the deferred byte beside byte 7
    uint32_t defer2 = 7, slack = 0;                             // PLANES == 5: defer < defer2 <= 6, and the deferred minima's sum
    if (PLANES == 5) {
        const uint32_t sel = plane_sel[2u * it.table];
        defer2 = min(max(sel >> 4, 1u), 6u);                    // (whatever the bytes hold, the plane offsets stay inside a tile)
        defer = min(sel & 15u, defer2 - 1u);
        slack = min((uint32_t)plane_sel[2u * it.table + 1u], 127u);
        build_pair_tables<16, 5>(qtables + (uint64_t)it.table * 256, defer, defer2);
    } else if (PLANES == 6) {
        defer = min((uint32_t)plane_sel[it.table], 6u);
        build_pair_tables<16, 6>(qtables + (uint64_t)it.table * 256, defer);
    } else {
        build_pair_tables<16>(qtables + (uint64_t)it.table * 256);
    }
    const uint32_t bound = prefix_bound(qs, it.order >> 16, R, reinterpret_cast<uint32_t*>(smem + C::HIST_OFF),
                                        reinterpret_cast<uint32_t*>(smem + C::BOUND_OFF));

    const uint32_t tid = threadIdx.x;
    const uint32_t lane_lo = (tid & 31u) * 4u;
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    typedef const __attribute__((address_space(1))) u32x4* gvec_t;
    typedef const __attribute__((address_space(1))) u32x2* grow_t;
    typedef const __attribute__((address_space(1))) unsigned char* gbyte_t;
    const gvec_t planes = (gvec_t)(uintptr_t)it.split;
    const gbyte_t byte7 = (gbyte_t)(uintptr_t)(it.codes + 7);     // byte 7 of run code r at 8 r
    const grow_t rows = (grow_t)(uintptr_t)it.codes;              // run code r, all 8 bytes
    lds_base_is_zero();
    const uint32_t n = it.n;
    const uint32_t ntiles = (n + kSplitTile - 1) / kSplitTile;
    uint32_t first = blockIdx.x, last = ntiles, step = gridDim.x;
    if (CHUNK) {
        const uint32_t per = (ntiles + gridDim.x - 1) / gridDim.x;
        first = blockIdx.x * per;
        last = min(ntiles, first + per);
        step = 1;
    }
    const uint32_t tiles_full = n / kSplitTile;
    const uint32_t full_last = min(last, tiles_full);
    // vector offset of the plane streamed into slot b (uniform; PLANES == 7: b itself)
    uint32_t poff[PLANES];
#pragma unroll
    for (int b = 0; b < PLANES; ++b)
        poff[b] = (PLANES == 7 ? (uint32_t)b : split_byte<PLANES == 7 ? 6 : PLANES>(b, defer, defer2)) * (kSplitTile / 16);
    // a survivor has min(127, partial) < bsurv; 5 planes: the bound less the slack, 0 = no survivor (never wraps)
    const uint32_t bsurv = PLANES == 5 ? (bound > slack ? bound - slack : 0u) : bound;
    const uint32_t bound4 = bsurv * 0x01010101u;

    // survivors of the previous iteration: byte c of pend = min(127, partial) of the lane's code c, 0xff = none
    uint32_t pend[4] = {~0u, ~0u, ~0u, ~0u};
    uint32_t pend_base = 0;                                     // run index of the lane's code 0 in that iteration
    bool any_pend = false;
    // ... and after their deferred bytes: byte c of res = the candidate's value (< bound), 0xff = none
    uint32_t res[4];
    uint32_t res_base = 0;
    bool any_res = false;
    uint32_t nsurv = 0;

    auto resolve = [&]() __attribute__((always_inline)) {                                      // pend -> res
        if constexpr (PLANES <= 6) {
            // bit 8 k + w of m = code 4 w + k survives (bit 7 of its byte in pend[w] is clear)
            uint32_t m = ((~pend[0] & 0x80808080u) >> 7) | ((~pend[1] & 0x80808080u) >> 6) | ((~pend[2] & 0x80808080u) >> 5) |
                         ((~pend[3] & 0x80808080u) >> 4);
            if (surv) nsurv += (uint32_t)__builtin_popcount(m);
            while (m) {
                const uint32_t i = (uint32_t)__builtin_ctz(m);
                m &= m - 1u;
                const uint32_t w = i & 3u, sh = i & 24u;
                const u32x2 x = rows[pend_base + 4u * w + (sh >> 3)];
                const uint32_t pw = w == 0 ? pend[0] : w == 1 ? pend[1] : w == 2 ? pend[2] : pend[3];
                const uint64_t xw = (((uint64_t)x.y) << 32) | x.x;
                const uint32_t xd = (uint32_t)(xw >> (8u * defer)) & 0xffu;
                // the deferred bytes' slots PLANES..6 and slot 7 (byte 7): dword group 1 (+128), bytes 1 (5 planes only), 2 and 3
                uint32_t s = ((pw >> sh) & 0xffu) +
                             *reinterpret_cast<lds_bytes_t>(static_cast<uintptr_t>(((xd << 8) | lane_lo) + (PLANES == 5 ? 129u : 130u))) +
                             *reinterpret_cast<lds_bytes_t>(static_cast<uintptr_t>(((x.y >> 24 << 8) | lane_lo) + 131u));
                if constexpr (PLANES == 5) {
                    const uint32_t xd2 = (uint32_t)(xw >> (8u * defer2)) & 0xffu;
                    s += *reinterpret_cast<lds_bytes_t>(static_cast<uintptr_t>(((xd2 << 8) | lane_lo) + 130u));
                }
                const uint32_t cv = min(s, 127u);
                const uint32_t upd = (pw & ~(0xffu << sh)) | ((cv < bound ? cv : 0xffu) << sh);
#pragma unroll
                for (int u = 0; u < 4; ++u) pend[u] = w == (uint32_t)u ? upd : pend[u];
            }
#pragma unroll
            for (int w = 0; w < 4; ++w) res[w] = pend[w];
        } else {
            uint32_t x[16];                                     // (byte-7 loads all in flight together)
#pragma unroll
            for (int c = 0; c < 16; ++c) {
                x[c] = 0;
                if (((pend[c >> 2] >> (8 * (c & 3))) & 0xffu) != 0xffu) x[c] = byte7[(uint64_t)(pend_base + c) * 8u];
            }
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                uint32_t r = ~0u;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const uint32_t pv = (pend[w] >> (8 * k)) & 0xffu;
                    // P_7[x]: dword group g = 1 (+128), byte j = 3
                    const uint32_t s = pv + *reinterpret_cast<lds_bytes_t>(static_cast<uintptr_t>(((x[4 * w + k] << 8) | lane_lo) + 131u));
                    const uint32_t cv = min(s, 127u);
                    if (pv != 0xffu && cv < bound) r &= ~(0xffu << (8 * k)) | (cv << (8 * k));
                }
                res[w] = r;
            }
        }
        res_base = pend_base;
        any_res = (res[0] & res[1] & res[2] & res[3]) != ~0u;
    };
    auto emit_res = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            const uint32_t r = (res[c >> 2] >> (8 * (c & 3))) & 0xffu;
            if (r != 0xffu)
                emit_candidate(qs, hdr, out, cand_cap, it.labels, it.key_base, it.order, it.dup_pos, it.dup_reps,
                               it.pos0 + res_base + c, r);
        }
    };
    auto step_tile = [&](uint32_t t, auto full) __attribute__((always_inline)) {
        u32x4 v[PLANES];
        const uint32_t e0 = t * (kSplitBytes * kSplitTile / 16) + tid;     // vector index of plane 0
#pragma unroll
        for (int b = 0; b < PLANES; ++b)
            v[b] = NT ? __builtin_nontemporal_load(planes + e0 + poff[b]) : planes[e0 + poff[b]];
        if (__builtin_expect(any_pend, 0)) resolve();           // the previous iteration's survivors, behind this one's loads
        const uint32_t base = t * kSplitTile + tid * 16u;       // run index of the lane's code 0
        uint32_t cv[16];
        uint32_t best = 127u;
        if (PROBE) {
            u32x4 a = v[0];
#pragma unroll
            for (int b = 1; b < PLANES; ++b) a ^= v[b];
            const uint32_t s = a.x ^ a.y ^ a.z ^ a.w;
#pragma unroll
            for (int c = 0; c < 16; ++c) cv[c] = 127u;
            cv[0] = (s == 0x12345678u) ? 0u : 127u;
            best = cv[0];
        } else {
#pragma unroll
            for (int w = 0; w < 4; ++w) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    uint32_t s = 0;
#pragma unroll
                    for (int b = 0; b < PLANES; ++b) {
                        // byte0 = bank*4, byte1 = code byte k of the plane in slot b; table slot b at (b >> 2) * 128 + (b & 3)
                        const uint32_t a = __builtin_amdgcn_perm(v[b][w], lane_lo, 0x0c0c0000u | ((4u + k) << 8));
                        s += *reinterpret_cast<lds_bytes_t>(static_cast<uintptr_t>(a + (b >> 2) * 128 + (b & 3)));
                    }
                    uint32_t c = min(s, 127u);
                    if (!decltype(full)::value) c = base + 4 * w + k < n ? c : 127u;   // past the run's end: never < bound
                    cv[4 * w + k] = c;
                    best = min(best, c);
                }
            }
        }
        any_pend = false;
        if (__builtin_expect(best < bsurv, PLANES <= 6)) {      // 7 planes: rare; 6, 5: most wave iterations of a long level
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                if constexpr (PLANES <= 6) {
                    // bytes >= bsurv -> 0xff, four at a time (all bytes and bsurv are <= 127: no borrow crosses a byte)
                    const uint32_t p = cv[4 * w] | (cv[4 * w + 1] << 8) | (cv[4 * w + 2] << 16) | (cv[4 * w + 3] << 24);
                    const uint32_t ge = ((p | 0x80808080u) - bound4) & 0x80808080u;
                    pend[w] = p | ((ge >> 7) * 0xffu);
                } else {
                    uint32_t p = ~0u;
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (cv[4 * w + k] < bound) p &= ~(0xffu << (8 * k)) | (cv[4 * w + k] << (8 * k));
                    pend[w] = p;
                }
            }
            pend_base = base;
            any_pend = true;
        }
        if (__builtin_expect(any_res, 0)) {                     // the previous iteration's candidates
            emit_res();
            any_res = false;
        }
    };
    using full_t = std::integral_constant<bool, true>;
    using part_t = std::integral_constant<bool, false>;
    uint32_t t = first;
    for (; t < full_last; t += step) step_tile(t, full_t());
    for (; t < last; t += step) step_tile(t, part_t());
    if (any_pend) {
        resolve();
        if (any_res) emit_res();
    }
    if (PLANES <= 6 && surv) {                                  // (uniform) one global atomic per workgroup: the waves' counts meet in LDS
        uint32_t* cnt = reinterpret_cast<uint32_t*>(smem + C::HIST_OFF);
        __syncthreads();
        if (tid == 0) *cnt = 0;
        __syncthreads();
        const uint32_t tot = dpp_wave_incl_sum(nsurv);          // lane 63: the wave's count
        if ((tid & 63u) == 63u && tot) atomicAdd(cnt, tot);
        __syncthreads();
        if (tid == 0 && *cnt) atomicAdd(surv, (unsigned long long)*cnt);
    }
}

// ---------------------------------------------------------------------------------------------
// Nibble form of the split scan (16x4, one query per pass): the run is streamed from the partition's nibble-plane copy
// (kNibTileBytes per kSplitTile-code tile, launch_nib_copy), NS = 8, 9 or 10 of the 16 sub-quantizers per code, i.e. 4, 4.5
// or 5 of the 8 code bytes; which ones is the table's choice (plane_choice_nib: any of the 16, byte 7's two included).
//   Table entries are >= 0, so the sum over the streamed sub-quantizers is a lower bound of the code's value, and with
//   c = min(127, the sum over the deferred s of min T[s]) every code's full sum is >= partial + c.  A code whose partial is
//   not below bound - c therefore cannot be a candidate: the survivor test is min(127, partial) < bsurv = bound > c ? bound - c : 0
//   (0: no code survives).  A survivor reads its row-major 8-byte word, adds the deferred sub-quantizers' entries from the
//   plain int8 table in LDS (the staging copy; bank conflicts do not matter there) and is emitted when min(127, full) < bound:
//   the candidates are those of scan_i8_kernel.  The argument holds for ANY deferred set as long as c is a lower bound of the
//   deferred entries' sum; the kernel derives the streamed list and its complement, the deferred set, from the choice bytes
//   itself (nib_streamed: always NS distinct sub-quantizers, whatever the bytes hold), so only a wrong c could lose a
//   candidate, and c is clamped to 127 as in the 5-plane form.
//   Loop: the 5-plane form's.  A lane holds 16 codes per iteration: one 8-byte load per streamed plane (two dwords of eight
//   codes each: codes 0-3 in the low nibbles of bytes 0-3, codes 4-7 in the high nibbles).  Two planes A, B merge into the
//   byte indices of a pair table P[x] = T[a][x & 15] + T[b][x >> 4] with two bit-field inserts per eight codes:
//   (A & 0x0f0f0f0f) | (B << 4 & 0xf0f0f0f0) for codes 0-3, (A >> 4 & 0x0f0f0f0f) | (B & 0xf0f0f0f0) for codes 4-7.  An odd
//   NS leaves one single plane, which has two table slots, T[a][x & 15] and T[a][x >> 4], and so needs no mask: NS / 2 + (NS & 1)
//   lookups per code.  The image is built permuted (build_nib_tables) with the bank replication of build_pair_tables.
//   Survivors are packed, tested, resolved one iteration late and emitted exactly as with 5 planes.
// PROBE: XOR of the streamed planes (the streaming ceiling of this form; results meaningless).
// surv (profile option only, else null): survivor count, one atomicAdd per workgroup at exit.
// ---------------------------------------------------------------------------------------------
// The NS streamed sub-quantizers of a table as nibbles of a 64-bit list, from its deferred mask: the clear bits in ascending
// order, cyclically, from the one behind the highest deferred sub-quantizer on (so an odd NS's single plane, the last of the
// list, can be any of the 16), then (a mask with more than 16 - NS bits set: never written by plane_choice_nib) set bits in the
// same order until there are NS.  used = the list as a bit set; its complement is the deferred set the kernel works with.
template <int NS>
__device__ __forceinline__ uint64_t nib_streamed(uint32_t mask, uint32_t& used) {
    mask &= 0xffffu;
    const uint32_t start = mask ? 32u - (uint32_t)__builtin_clz(mask) : 0u;
    uint64_t list = 0;
    uint32_t cnt = 0;
    used = 0;
#pragma unroll
    for (uint32_t pass = 0; pass < 2; ++pass)
#pragma unroll
        for (uint32_t i = 0; i < 16; ++i) {
            const uint32_t s = (start + i) & 15u;
            if (((mask >> s) & 1u) == pass && cnt < (uint32_t)NS) {
                list |= (uint64_t)s << (4u * cnt);
                used |= 1u << s;
                ++cnt;
            }
        }
    return list;
}

// build_pair_tables for the nibble form: slot p < NS / 2 of the image holds the pair table of the streamed sub-quantizers
// 2p and 2p + 1 of the list; NS odd: slot NS / 2 = T[last][x & 15], slot NS / 2 + 1 = T[last][x >> 4]; other slots 0.
// The staging copy of the int8 table (ScanCfg::STAGE_OFF) stays in LDS for the survivors' deferred entries.
template <int NS>
__device__ __forceinline__ void build_nib_tables(const int8_t* __restrict__ qt, uint64_t list) {
    using C = ScanCfg<16>;
    constexpr uint32_t NP = NS / 2;
    const int t = threadIdx.x;
    if (t < 64) reinterpret_cast<uint32_t*>(smem + C::STAGE_OFF)[t] = reinterpret_cast<const uint32_t*>(qt)[t];
    __syncthreads();
    const unsigned char* T = smem + C::STAGE_OFF;
    constexpr int kIter = C::TABLE_BYTES / 16 / kWG;
    const uint32_t lane = (uint32_t)t & 63u, wave = (uint32_t)t >> 6;
    uint32_t w = 0;
    {
        const uint32_t pi = lane & (8u * kIter - 1u);
        const uint32_t k = pi >> 3, within = pi & 7u;
        const uint32_t x = (k & 3u) * 64u + wave * 4u + (within >> 1);
        const uint32_t g = (k >> 2) * 2u + (within & 1u);
        const uint32_t last = (uint32_t)(list >> (4u * (NS - 1))) & 15u;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t slot = 4u * g + j;
            uint32_t ra = 0, rb = 0, ma = 0, mb = 0;
            if (slot < NP) {
                ra = (uint32_t)(list >> (8u * slot)) & 15u;
                rb = (uint32_t)(list >> (8u * slot + 4u)) & 15u;
                ma = mb = 1;
            } else if ((NS & 1) && slot == NP) {
                ra = last;
                ma = 1;
            } else if ((NS & 1) && slot == NP + 1u) {
                rb = last;
                mb = 1;
            }
            const uint32_t v = (uint32_t)T[ra * 16u + (x & 15u)] * ma + (uint32_t)T[rb * 16u + (x >> 4)] * mb;
            w |= v << (8u * j);
        }
    }
#pragma unroll
    for (int k = 0; k < kIter; ++k) {
        const uint32_t wk = (uint32_t)__builtin_amdgcn_ds_bpermute((int)((k * 8u + (lane >> 3)) * 4u), (int)w);
        *reinterpret_cast<uint4*>(smem + ((size_t)k * kWG + t) * 16) = make_uint4(wk, wk, wk, wk);
    }
}

template <int NS, bool NT, bool CHUNK, bool PROBE>
__global__ __launch_bounds__(kWG, 8) void scan_i8_nib_kernel(
    const ScanItem* __restrict__ items, const int8_t* __restrict__ qtables, QueryState* __restrict__ qstates,
    CandHeader* __restrict__ hdr, Cand* __restrict__ out, uint32_t cand_cap, uint32_t R,
    const uint8_t* __restrict__ nib_sel, unsigned long long* __restrict__ surv) {
    static_assert(NS >= 8 && NS <= 10, "8, 9 or 10 of the 16 nibble planes");
    static_assert(kSplitTile == 16u * kWG, "a workgroup iteration is one tile: 16 codes per lane");
    using C = ScanCfg<16>;
    constexpr int NP = NS / 2;                                  // fused pairs
    constexpr bool ODD = (NS & 1) != 0;                         // ... and one single plane
    const ScanItem it = items[blockIdx.y];
    QueryState* qs = qstates + it.query;
    out += (uint64_t)it.query * cand_cap;
    const uint8_t* sel = nib_sel + (size_t)it.table * kNibSelBytes + 4u * (NS - 8);
    const uint32_t slack = min((uint32_t)sel[2], 127u);
    uint32_t used;
    const uint64_t list = nib_streamed<NS>((uint32_t)sel[0] | ((uint32_t)sel[1] << 8), used);
    const uint32_t defmask = 0xffffu & ~used;                   // (whatever the bytes hold: the complement of what is streamed)
    build_nib_tables<NS>(qtables + (uint64_t)it.table * 256, list);
    const uint32_t bound = prefix_bound(qs, it.order >> 16, R, reinterpret_cast<uint32_t*>(smem + C::HIST_OFF),
                                        reinterpret_cast<uint32_t*>(smem + C::BOUND_OFF));

    const uint32_t tid = threadIdx.x;
    const uint32_t lane_lo = (tid & 31u) * 4u;
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    typedef const __attribute__((address_space(1))) u32x2* gvec_t;
    const gvec_t planes = (gvec_t)(uintptr_t)it.split;          // (a launch of this form: the tile in the nibble-plane copy)
    const gvec_t rows = (gvec_t)(uintptr_t)it.codes;            // run code r, all 8 bytes
    lds_base_is_zero();
    const uint32_t n = it.n;
    const uint32_t ntiles = (n + kSplitTile - 1) / kSplitTile;
    uint32_t first = blockIdx.x, last = ntiles, step = gridDim.x;
    if (CHUNK) {
        const uint32_t per = (ntiles + gridDim.x - 1) / gridDim.x;
        first = blockIdx.x * per;
        last = min(ntiles, first + per);
        step = 1;
    }
    const uint32_t tiles_full = n / kSplitTile;
    const uint32_t full_last = min(last, tiles_full);
    // 8-byte-vector offset of the plane streamed i-th (uniform; a sub-quantizer is 0..15: inside the tile)
    uint32_t poff[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) poff[i] = ((uint32_t)(list >> (4 * i)) & 15u) * (kSplitTile / 16);
    const uint32_t bsurv = bound > slack ? bound - slack : 0u;  // 0 = no survivor (never wraps)
    const uint32_t bound4 = bsurv * 0x01010101u;

    // survivors of the previous iteration: byte k of pend[w] = min(127, partial) of the lane's code 4 w + k, 0xff = none
    uint32_t pend[4] = {~0u, ~0u, ~0u, ~0u};
    uint32_t pend_base = 0;
    bool any_pend = false;
    uint32_t res[4];
    uint32_t res_base = 0;
    bool any_res = false;
    uint32_t nsurv = 0;

    auto resolve = [&]() __attribute__((always_inline)) {                                      // pend -> res
        // bit 8 k + w of m = code 4 w + k survives (bit 7 of its byte in pend[w] is clear)
        uint32_t m = ((~pend[0] & 0x80808080u) >> 7) | ((~pend[1] & 0x80808080u) >> 6) | ((~pend[2] & 0x80808080u) >> 5) |
                     ((~pend[3] & 0x80808080u) >> 4);
        if (surv) nsurv += (uint32_t)__builtin_popcount(m);
        while (m) {
            const uint32_t i = (uint32_t)__builtin_ctz(m);
            m &= m - 1u;
            const uint32_t w = i & 3u, sh = i & 24u;
            const u32x2 x = rows[pend_base + 4u * w + (sh >> 3)];
            const uint32_t pw = w == 0 ? pend[0] : w == 1 ? pend[1] : w == 2 ? pend[2] : pend[3];
            const uint64_t xw = (((uint64_t)x.y) << 32) | x.x;
            uint32_t s = (pw >> sh) & 0xffu;
            for (uint32_t dm = defmask; dm; dm &= dm - 1u) {    // (uniform trip count) the deferred sub-quantizers' entries
                const uint32_t sq = (uint32_t)__builtin_ctz(dm);
                s += smem[C::STAGE_OFF + 16u * sq + ((uint32_t)(xw >> (4u * sq)) & 15u)];
            }
            const uint32_t cv = min(s, 127u);
            const uint32_t upd = (pw & ~(0xffu << sh)) | ((cv < bound ? cv : 0xffu) << sh);
#pragma unroll
            for (int u = 0; u < 4; ++u) pend[u] = w == (uint32_t)u ? upd : pend[u];
        }
#pragma unroll
        for (int w = 0; w < 4; ++w) res[w] = pend[w];
        res_base = pend_base;
        any_res = (res[0] & res[1] & res[2] & res[3]) != ~0u;
    };
    auto emit_res = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            const uint32_t r = (res[c >> 2] >> (8 * (c & 3))) & 0xffu;
            if (r != 0xffu)
                emit_candidate(qs, hdr, out, cand_cap, it.labels, it.key_base, it.order, it.dup_pos, it.dup_reps,
                               it.pos0 + res_base + c, r);
        }
    };
    auto step_tile = [&](uint32_t t, auto full) __attribute__((always_inline)) {
        u32x2 v[NS];
        const uint32_t e0 = t * (kNibTileBytes / 8) + tid;      // vector index of plane 0 (t < 2^17: no wrap)
#pragma unroll
        for (int i = 0; i < NS; ++i)
            v[i] = NT ? __builtin_nontemporal_load(planes + e0 + poff[i]) : planes[e0 + poff[i]];
        if (__builtin_expect(any_pend, 0)) resolve();           // the previous iteration's survivors, behind this one's loads
        const uint32_t base = t * kSplitTile + tid * 16u;       // run index of the lane's code 0
        uint32_t cv[16];
        uint32_t best = 127u;
        if (PROBE) {
            u32x2 a = v[0];
#pragma unroll
            for (int i = 1; i < NS; ++i) a ^= v[i];
#pragma unroll
            for (int c = 0; c < 16; ++c) cv[c] = 127u;
            cv[0] = ((a.x ^ a.y) == 0x12345678u && base < n) ? 0u : 127u;
            best = cv[0];
        } else {
            constexpr uint32_t LO = 0x0f0f0f0fu;
#pragma unroll
            for (int w = 0; w < 2; ++w) {
                uint32_t idx[2][NP];                            // [codes 0-3 | 4-7 of the dword's eight][pair]: four byte indices each
#pragma unroll
                for (int p = 0; p < NP; ++p) {
                    const uint32_t A = v[2 * p][w], B = v[2 * p + 1][w];
                    idx[0][p] = (A & LO) | ((B << 4) & ~LO);
                    idx[1][p] = ((A >> 4) & LO) | (B & ~LO);
                }
#pragma unroll
                for (int h = 0; h < 2; ++h) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        uint32_t s = 0;
#pragma unroll
                        for (int p = 0; p < NP; ++p) {
                            // byte0 = bank*4, byte1 = byte k of the merged index; table slot p at (p >> 2) * 128 + (p & 3)
                            const uint32_t a = __builtin_amdgcn_perm(idx[h][p], lane_lo, 0x0c0c0000u | ((4u + k) << 8));
                            s += *reinterpret_cast<lds_bytes_t>(static_cast<uintptr_t>(a + (p >> 2) * 128 + (p & 3)));
                        }
                        if (ODD) {                              // the single plane: slot NP reads the low nibble, slot NP + 1 the high one
                            constexpr int sl = NP + 0;
                            const uint32_t a = __builtin_amdgcn_perm(v[NS - 1][w], lane_lo, 0x0c0c0000u | ((4u + k) << 8));
                            s += *reinterpret_cast<lds_bytes_t>(static_cast<uintptr_t>(a + ((sl + h) >> 2) * 128 + ((sl + h) & 3)));
                        }
                        uint32_t c = min(s, 127u);
                        if (!decltype(full)::value) c = base + 8 * w + 4 * h + k < n ? c : 127u;   // past the run's end: never < bound
                        cv[8 * w + 4 * h + k] = c;
                        best = min(best, c);
                    }
                }
            }
        }
        any_pend = false;
        if (__builtin_expect(best < bsurv, 1)) {                // most wave iterations of a long level
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                // bytes >= bsurv -> 0xff, four at a time (all bytes and bsurv are <= 127: no borrow crosses a byte)
                const uint32_t p = cv[4 * w] | (cv[4 * w + 1] << 8) | (cv[4 * w + 2] << 16) | (cv[4 * w + 3] << 24);
                const uint32_t ge = ((p | 0x80808080u) - bound4) & 0x80808080u;
                pend[w] = p | ((ge >> 7) * 0xffu);
            }
            pend_base = base;
            any_pend = true;
        }
        if (__builtin_expect(any_res, 0)) {                     // the previous iteration's candidates
            emit_res();
            any_res = false;
        }
    };
    using full_t = std::integral_constant<bool, true>;
    using part_t = std::integral_constant<bool, false>;
    uint32_t t = first;
    for (; t < full_last; t += step) step_tile(t, full_t());
    for (; t < last; t += step) step_tile(t, part_t());
    if (any_pend) {
        resolve();
        if (any_res) emit_res();
    }
    if (surv) {                                                 // (uniform) one global atomic per workgroup: the waves' counts meet in LDS
        uint32_t* cnt = reinterpret_cast<uint32_t*>(smem + C::HIST_OFF);
        __syncthreads();
        if (tid == 0) *cnt = 0;
        __syncthreads();
        const uint32_t tot = dpp_wave_incl_sum(nsurv);          // lane 63: the wave's count
        if ((tid & 63u) == 63u && tot) atomicAdd(cnt, tot);
        __syncthreads();
        if (tid == 0 && *cnt) atomicAdd(surv, (unsigned long long)*cnt);
    }
}

// ---------------------------------------------------------------------------------------------
// Bucket form of the split scan (16x4, one query per pass): the run is streamed from the partition's bucket copy
// (host/level_plan.hpp: kBktTileBytes per kSplitTile-slot tile, launch_bkt_*), in which every 16-slot lane group holds codes of
// ONE key = code bytes 0 and 1, i.e. sub-quantizers 0-3.  A lane loads its group's uint16 id and NSP = 4, 5, 6 or 7 of the 12
// nibble planes of sub-quantizers 4-15 (which: the table's choice, plane_choice_bkt): 2 bytes per 16 codes for four
// sub-quantizers instead of 2 bytes per code.
//   The partial sum starts from P01[id & 255] + P23[id >> 8], the pair tables of rows 0-3 (slots 0 and 1 of the LDS image):
//   those four rows are EXACT.  The paid rows are exact too, and with c = min(127, the sum over the deferred s of min T[s]) every
//   code's full sum is >= partial + c: the survivor test is the nibble form's, min(127, partial) < bsurv = bound > c ? bound - c : 0.
//   A survivor reads its slot's 8-byte code from the side array, adds the deferred rows' entries from the staged int8 table and
//   is a candidate when min(127, full) < bound.  A candidate reads perm[slot], its position in the partition; a padding slot
//   (kBktPad: a copy of a code that has a real slot of its own) is dropped, every other one goes to emit_candidate with that
//   position.  A block of the copy lies inside one bound level and a run covers whole blocks, so the run's slots hold exactly
//   the codes of the row-major run: the candidate set is that of scan_i8_kernel, in another order, and the stream is sorted
//   by position before the replay.
//   Loop: the nibble form's (two planes merge into pair-table indices; an odd NSP leaves one single plane with two slots);
//   a run is whole tiles, so there is no ragged end.
// PROBE: XOR of the streamed planes and the id (the streaming ceiling of this form; results meaningless).
// surv (profile option only, else null): survivor count (padding slots included), one atomicAdd per workgroup at exit.
// ---------------------------------------------------------------------------------------------
// The list build_nib_tables takes, NSP + 4 nibbles: sub-quantizers 0-3 (slots 0 and 1: the free pair tables), then the NSP
// paid ones: the clear bits of the deferred mask among 4..15, ascending, then (a mask with more than 12 - NSP bits set: never
// written by plane_choice_bkt) set bits until there are NSP.  used = the list as a bit set; its complement is the deferred set.
template <int NSP>
__device__ __forceinline__ uint64_t bkt_streamed(uint32_t mask, uint32_t& used) {
    mask &= 0xfff0u;
    uint64_t list = 0x3210ull;
    uint32_t cnt = 4;
    used = 0xfu;
#pragma unroll
    for (uint32_t pass = 0; pass < 2; ++pass)
#pragma unroll
        for (uint32_t s = 4; s < 16; ++s)
            if (((mask >> s) & 1u) == pass && cnt < (uint32_t)NSP + 4u) {
                list |= (uint64_t)s << (4u * cnt);
                used |= 1u << s;
                ++cnt;
            }
    return list;
}

// The wide form's lists (FREE = 5): the NSP paid sub-quantizers among 5..15 as nibbles of `paid` (the clear bits of the deferred
// mask, ascending, then set bits until there are NSP), and the list build_nib_tables takes.  An even NSP: 0-3, the paid ones, then
// row 4 as the single row at the end (its low-nibble slot is T4).  An odd NSP: 0-3, then row 4 FUSED with the first paid plane
// into a pair table, then the other paid pairs.  used = the rows the loop sums; its complement is the deferred set.
template <int NSP>
__device__ __forceinline__ uint64_t bktw_streamed(uint32_t mask, uint32_t& used, uint64_t& paid) {
    mask &= 0xffe0u;
    paid = 0;
    uint32_t cnt = 0;
    used = 0x1fu;
#pragma unroll
    for (uint32_t pass = 0; pass < 2; ++pass)
#pragma unroll
        for (uint32_t s = 5; s < 16; ++s)
            if (((mask >> s) & 1u) == pass && cnt < (uint32_t)NSP) {
                paid |= (uint64_t)s << (4u * cnt);
                used |= 1u << s;
                ++cnt;
            }
    return (NSP & 1) ? (0x43210ull | (paid << 20)) : (0x3210ull | (paid << 16) | (4ull << (4u * (NSP + 4))));
}

// The body of both bucket kernels.  FREE = 4: narrow blocks (16-bit key, 12 planes of sub-quantizers 4-15, NSP = 4..7 of them
// paid).  FREE = 5: wide octaves (20-bit key, 11 planes of sub-quantizers 5-15, NSP = 3..6 paid; the group's sub-quantizer 4 is
// one more byte of its id: s0 = P01[id & 255] + P23[id >> 8] + T4[id4], or, NSP odd, row 4 joins the first paid plane's pair table
// with id4 splatted into the low nibbles of the merged index).  sel = the form's choice bytes of every table.
// Depth of the id ring of the PRUNE tile loop (below): the ids of a workgroup's tiles are requested this many tiles ahead.  1, 2 and 3
// were measured (profiles/r15_bktw_loop.txt); 3 takes the QUARTER kernels past 64 VGPRs.  With 2 those kernels stand at 62 - 63 of the
// 64 VGPRs that 8 waves per SIMD allow (58 - 59 before the ring): one more live value in scan_bkt_body costs scratch or occupancy, so
// read -Rpass-analysis=kernel-resource-usage after any change to it.  tests/test_gpu_bktw_prefetch.py reads the depth from the next
// line as it is written; keep its form.
constexpr uint32_t kBktwRing = 2;
template <int FREE, int NSP, bool NT, bool CHUNK, bool PROBE, bool PRUNE, bool QUARTER = false>
__device__ __forceinline__ void scan_bkt_body(
    const ScanItem* __restrict__ items, const int8_t* __restrict__ qtables, QueryState* __restrict__ qstates,
    CandHeader* __restrict__ hdr, Cand* __restrict__ out, uint32_t cand_cap, uint32_t R,
    const uint8_t* __restrict__ bkt_sel, unsigned long long* __restrict__ surv, unsigned long long* __restrict__ prune_cnt) {
    static_assert(FREE == 4 || FREE == 5, "16-bit or 20-bit key");
    static_assert(PRUNE || !QUARTER, "the quarter skip is a form of the group test");
    static_assert(FREE == 5 || (NSP >= 4 && NSP <= 7), "4, 5, 6 or 7 of the 12 paid nibble planes");
    static_assert(FREE == 4 || (NSP >= 3 && NSP <= 6), "3, 4, 5 or 6 of the 11 paid nibble planes");
    static_assert(kSplitTile == 16u * kWG, "a workgroup iteration is one tile: 16 slots per lane");
    static_assert(kBktTileBytes % 8 == 0 && kBktIdOff % 8 == 0, "8-byte plane vectors");
    static_assert(kBktwTileBytes % 8 == 0 && kBktwIdOff % 8 == 0, "8-byte plane vectors");
    using C = ScanCfg<16>;
    constexpr bool WIDE = FREE == 5;
    constexpr bool FUSE = WIDE && (NSP & 1) != 0;               // row 4 and the first paid plane share a pair table
    constexpr int NVP = NSP + (FUSE ? 1 : 0);                   // planes of the pair loop (FUSE: the first is the splatted id4)
    constexpr int NS = NSP + FREE;                              // rows in the LDS image
    constexpr int NP = NVP / 2;                                 // fused paid pairs: slots 2 .. 2 + NP - 1
    constexpr bool ODD = !WIDE && (NSP & 1) != 0;               // ... and one single plane: slots 2 + NP and 3 + NP
    static_assert(2 + NP + (ODD || (WIDE && !FUSE) ? 2 : 0) <= 8, "the LDS image has 8 slots");
    constexpr uint32_t kTile = WIDE ? kBktwTileBytes : kBktTileBytes, kIdOff = WIDE ? kBktwIdOff : kBktIdOff;
    const ScanItem it = items[blockIdx.y];
    QueryState* qs = qstates + it.query;
    out += (uint64_t)it.query * cand_cap;
    const uint8_t* sel = bkt_sel + (size_t)it.table * (WIDE ? kBktwSelBytes : kBktSelBytes) + 4u * (NSP - (WIDE ? 3 : 4));
    const uint32_t slack = min((uint32_t)sel[2], 127u);
    uint32_t used;
    uint64_t paid = 0;
    uint64_t list;
    if constexpr (WIDE) {
        list = bktw_streamed<NSP>((uint32_t)sel[0] | ((uint32_t)sel[1] << 8), used, paid);
    } else {
        list = bkt_streamed<NSP>((uint32_t)sel[0] | ((uint32_t)sel[1] << 8), used);
        paid = list >> 16;
    }
    const uint32_t defmask = 0xffffu & ~used;                   // (whatever the bytes hold: the complement of what is summed in the loop)
    build_nib_tables<NS>(qtables + (uint64_t)it.table * 256, list);
    const uint32_t bound = prefix_bound(qs, it.order >> 16, R, reinterpret_cast<uint32_t*>(smem + C::HIST_OFF),
                                        reinterpret_cast<uint32_t*>(smem + C::BOUND_OFF));

    const uint32_t tid = threadIdx.x;
    const uint32_t lane_lo = (tid & 31u) * 4u;
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    typedef const __attribute__((address_space(1))) u32x2* gvec_t;
    typedef const __attribute__((address_space(1))) unsigned short* gid_t;
    typedef const __attribute__((address_space(1))) unsigned char* gbyte_t;
    const gvec_t planes = (gvec_t)(uintptr_t)it.split;          // the run's first tile of the bucket copy
    const gid_t ids = (gid_t)(uintptr_t)(it.split + kIdOff) + tid;
    [[maybe_unused]] const gbyte_t id4s = (gbyte_t)(uintptr_t)(it.split + kBktwId4Off) + tid;   // (WIDE only)
    const gbyte_t side = (gbyte_t)(uintptr_t)it.codes;          // ... and of its side array
    lds_base_is_zero();
    const uint32_t ntiles = it.n / kSplitTile;                  // (n = slots: whole tiles)
    uint32_t first = blockIdx.x, last = ntiles, step = gridDim.x;
    if (CHUNK) {
        const uint32_t per = (ntiles + gridDim.x - 1) / gridDim.x;
        first = blockIdx.x * per;
        last = min(ntiles, first + per);
        step = 1;
    }
    // 8-byte-vector offset of the paid plane streamed i-th (uniform; sub-quantizer FREE..15: plane 0..15 - FREE, inside the tile)
    uint32_t poff[NSP];
#pragma unroll
    for (int i = 0; i < NSP; ++i)
        poff[i] = (((uint32_t)(paid >> (4 * i)) & 15u) - (uint32_t)FREE) % (WIDE ? kBktwPlanes : kBktPlanes) * (kSplitTile / 16);
    const uint32_t bsurv = bound > slack ? bound - slack : 0u;  // 0 = no survivor (never wraps)
    const uint32_t bound4 = bsurv * 0x01010101u;
    // PRUNE: pmin = the sum over the rows the pair loop adds (the paid ones and, FUSE, row 4) of min T[s], from the staged int8
    // table (build_nib_tables' barrier is behind us).  With s0 = the rows the loop starts from, every slot of a lane group has
    // partial >= s0 + pmin, so s0 + pmin >= bsurv means min(127, partial) >= bsurv in all 16: no survivor, and the group needs
    // neither its planes nor its pair lookups (bsurv <= 127; 32-bit sums: s0 <= 5 x 127, pmin <= 7 x 127; bsurv = 0 keeps nothing).
    [[maybe_unused]] uint32_t pmin = 0;
    if constexpr (PRUNE) {
        auto row_min = [&](uint32_t sq) __attribute__((always_inline)) {
            const uint32_t* row = reinterpret_cast<const uint32_t*>(smem + C::STAGE_OFF + 16u * sq);
            uint32_t m = 255u;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t x = row[j];
                m = min(min(m, x & 0xffu), min((x >> 8) & 0xffu, min((x >> 16) & 0xffu, x >> 24)));
            }
            return m;
        };
#pragma unroll
        for (int i = 0; i < NSP; ++i) pmin += row_min((uint32_t)(paid >> (4 * i)) & 15u);
        if constexpr (FUSE) pmin += row_min(4u);
    }
    // (wave-uniform) PRUNE: wave iterations skipped, lane groups pruned and, QUARTER, quarters of run iterations without a load
    [[maybe_unused]] uint32_t nskip = 0, npruned = 0, nquart = 0;

    // survivors of the previous iteration: byte k of pend[w] = min(127, partial) of the lane's slot 4 w + k, 0xff = none
    uint32_t pend[4] = {~0u, ~0u, ~0u, ~0u};
    uint32_t pend_base = 0;                                     // run slot of the lane's slot 0 in that iteration
    bool any_pend = false;
    uint32_t res[4];
    uint32_t res_base = 0;
    bool any_res = false;
    uint32_t nsurv = 0;

    // byte offset of run slot sl's tile in the side array (sl < 2^32: at most 2^18 tiles)
    auto side_tile = [&](uint32_t sl) __attribute__((always_inline)) { return (uint64_t)(sl / kSplitTile) * kBktSideBytes; };
    auto resolve = [&]() __attribute__((always_inline)) {                                      // pend -> res
        uint32_t m = ((~pend[0] & 0x80808080u) >> 7) | ((~pend[1] & 0x80808080u) >> 6) | ((~pend[2] & 0x80808080u) >> 5) |
                     ((~pend[3] & 0x80808080u) >> 4);
        if (surv) nsurv += (uint32_t)__builtin_popcount(m);
        const gbyte_t rows = side + side_tile(pend_base) + (uint64_t)(pend_base % kSplitTile) * 8u;   // the lane's 16 slot codes
        while (m) {
            const uint32_t i = (uint32_t)__builtin_ctz(m);
            m &= m - 1u;
            const uint32_t w = i & 3u, sh = i & 24u;
            const u32x2 x = *(gvec_t)(rows + (4u * w + (sh >> 3)) * 8u);
            const uint32_t pw = w == 0 ? pend[0] : w == 1 ? pend[1] : w == 2 ? pend[2] : pend[3];
            const uint64_t xw = (((uint64_t)x.y) << 32) | x.x;
            uint32_t s = (pw >> sh) & 0xffu;
            for (uint32_t dm = defmask; dm; dm &= dm - 1u) {    // (uniform trip count) the deferred sub-quantizers' entries
                const uint32_t sq = (uint32_t)__builtin_ctz(dm);
                s += smem[C::STAGE_OFF + 16u * sq + ((uint32_t)(xw >> (4u * sq)) & 15u)];
            }
            const uint32_t cv = min(s, 127u);
            const uint32_t upd = (pw & ~(0xffu << sh)) | ((cv < bound ? cv : 0xffu) << sh);
#pragma unroll
            for (int u = 0; u < 4; ++u) pend[u] = w == (uint32_t)u ? upd : pend[u];
        }
#pragma unroll
        for (int w = 0; w < 4; ++w) res[w] = pend[w];
        res_base = pend_base;
        any_res = (res[0] & res[1] & res[2] & res[3]) != ~0u;
    };
    auto emit_res = [&]() __attribute__((always_inline)) {
        typedef const __attribute__((address_space(1))) uint32_t* gperm_t;
        const gperm_t perm = (gperm_t)(side + side_tile(res_base) + kBktPermOff) + res_base % kSplitTile;
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            const uint32_t r = (res[c >> 2] >> (8 * (c & 3))) & 0xffu;
            if (r != 0xffu) {
                const uint32_t pos = perm[c];                   // position in the partition; a padding slot is a copy: dropped
                if (pos != kBktPad)
                    emit_candidate(qs, hdr, out, cand_cap, it.labels, it.key_base, it.order, it.dup_pos, it.dup_reps, pos, r);
            }
        }
    };
    // the lane group's id of tile t (and, WIDE, its sub-quantizer 4).  id4 is the RAW byte: its users mask it (free_rows, the FUSE
    // splat).  A mask here sits between the load and the back edge of the PRUNE loop, which carries the value, and with it a wait for
    // the NEXT tile's id4 at the top of every iteration, before this tile's decision and plane loads.
    auto load_ids = [&](uint32_t t, uint32_t& id, uint32_t& id4) __attribute__((always_inline)) {
        const gid_t idp = ids + (uint64_t)t * (kTile / 2);
        id = NT ? __builtin_nontemporal_load(idp) : *idp;
        id4 = 0;
        if constexpr (WIDE) {
            const gbyte_t p4 = id4s + (uint64_t)t * kTile;
            id4 = NT ? __builtin_nontemporal_load(p4) : *p4;
        }
    };
    // the rows the pair loop starts from: P01[id & 255] in slot 0, P23[id >> 8] in slot 1 and, WIDE with an even NSP, the fifth free
    // row: the single row's low-nibble slot, T4[x & 15] (FUSE: row 4 is in the first pair table, not here)
    auto free_rows = [&](uint32_t id, uint32_t id4) __attribute__((always_inline)) {
        uint32_t s0 = *reinterpret_cast<lds_bytes_t>(static_cast<uintptr_t>((((id & 0xffu) << 8) | lane_lo) + 0u)) +
                      *reinterpret_cast<lds_bytes_t>(static_cast<uintptr_t>((((id >> 8) & 0xffu) << 8 | lane_lo) + 1u));
        if constexpr (WIDE && !FUSE) {
            constexpr int sl = NP + 2;
            s0 += *reinterpret_cast<lds_bytes_t>(static_cast<uintptr_t>((((id4 & 15u) << 8) | lane_lo) + (sl >> 2) * 128 + (sl & 3)));
        }
        return s0;
    };
    // PRUNE: pid / pid4 = the tile's ids, loaded kBktwRing iterations early, so that the decision comes before the plane loads
    auto step_tile = [&](uint32_t t, [[maybe_unused]] uint32_t pid, [[maybe_unused]] uint32_t pid4) __attribute__((always_inline)) {
        u32x2 v[NSP];
        const uint32_t e0 = t * (kTile / 8) + tid;              // vector index of plane 0 (t < 2^18: no wrap)
        uint32_t id, id4;                                       // (id4: WIDE, the group's sub-quantizer 4)
        [[maybe_unused]] uint32_t s0p = 0;
        bool run = true;                                        // (uniform) PRUNE: some lane of the wave keeps its group
        [[maybe_unused]] bool mine = true;                      // QUARTER: some lane of this lane's aligned 16-lane quarter does
        if constexpr (PRUNE) {
            id = pid;
            id4 = pid4;
            s0p = free_rows(id, id4);
            const uint64_t keep = __builtin_amdgcn_ballot_w64(s0p + pmin < bsurv);   // lanes whose group may hold a survivor
            npruned += 64u - (uint32_t)__builtin_popcountll(keep);
            run = keep != 0;                                    // no lane keeps: an iteration with no survivor, without its loads and lookups
            nskip += run ? 0u : 1u;
            if constexpr (QUARTER) {
                // a quarter reads 128 contiguous, 128-byte-aligned bytes of each plane: one none of whose lanes keeps loads nothing
                mine = ((uint32_t)(keep >> (tid & 48u)) & 0xffffu) != 0;
                uint32_t idle = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) idle += ((uint32_t)(keep >> (16 * j)) & 0xffffu) == 0 ? 1u : 0u;
                nquart += run ? idle : 0u;
            }
        } else {
            load_ids(t, id, id4);
        }
        if (run) {
#pragma unroll
            for (int i = 0; i < NSP; ++i) v[i] = u32x2{0u, 0u};  // (QUARTER: what a lane of a quarter without a load presents)
            if (!QUARTER || mine) {
#pragma unroll
                for (int i = 0; i < NSP; ++i)
                    v[i] = NT ? __builtin_nontemporal_load(planes + e0 + poff[i]) : planes[e0 + poff[i]];
            }
        }
        if (__builtin_expect(any_pend, 0)) resolve();           // the previous iteration's survivors, behind this one's loads
        if (!run) {
            // as after an iteration with no survivor: that one leaves pend's bytes as resolve() wrote them too and clears the flag
            // only; pend is read under any_pend alone (resolve, the drain), res under any_res alone
            any_pend = false;
        } else {
        const uint32_t base = t * kSplitTile + tid * 16u;       // run slot of the lane's slot 0
        uint32_t cv[16];
        uint32_t best = 127u;
        if (PROBE) {
            u32x2 a = v[0];
#pragma unroll
            for (int i = 1; i < NSP; ++i) a ^= v[i];
#pragma unroll
            for (int c = 0; c < 16; ++c) cv[c] = 127u;
            cv[0] = ((a.x ^ a.y ^ id ^ ((id4 & 15u) << 16)) == 0x12345678u) ? 0u : 127u;
            best = cv[0];
        } else {
            constexpr uint32_t LO = 0x0f0f0f0fu;
            const uint32_t s0 = PRUNE ? s0p : free_rows(id, id4);   // the group's free rows
            [[maybe_unused]] const uint32_t id4s8 = (id4 & 15u) * 0x11111111u;   // FUSE: id4 in every nibble, the pair loop's plane 0
#pragma unroll
            for (int w = 0; w < 2; ++w) {
                uint32_t idx[2][NP > 0 ? NP : 1];               // [slots 0-3 | 4-7 of the dword's eight][pair]: four byte indices each
#pragma unroll
                for (int p = 0; p < NP; ++p) {
                    const uint32_t A = FUSE ? (p == 0 ? id4s8 : v[p > 0 ? 2 * p - 1 : 0][w]) : v[2 * p][w];
                    const uint32_t B = FUSE ? v[2 * p][w] : v[2 * p + 1][w];
                    idx[0][p] = (A & LO) | ((B << 4) & ~LO);
                    idx[1][p] = ((A >> 4) & LO) | (B & ~LO);
                }
#pragma unroll
                for (int h = 0; h < 2; ++h) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        uint32_t s = s0;
#pragma unroll
                        for (int p = 0; p < NP; ++p) {
                            // byte0 = bank*4, byte1 = byte k of the merged index; table slot sl = p + 2 at (sl >> 2) * 128 + (sl & 3)
                            const uint32_t a = __builtin_amdgcn_perm(idx[h][p], lane_lo, 0x0c0c0000u | ((4u + k) << 8));
                            s += *reinterpret_cast<lds_bytes_t>(static_cast<uintptr_t>(a + ((p + 2) >> 2) * 128 + ((p + 2) & 3)));
                        }
                        if (ODD) {                              // the single plane: its first slot reads the low nibble, the next one the high one
                            constexpr int sl = NP + 2;
                            const uint32_t a = __builtin_amdgcn_perm(v[NSP - 1][w], lane_lo, 0x0c0c0000u | ((4u + k) << 8));
                            s += *reinterpret_cast<lds_bytes_t>(static_cast<uintptr_t>(a + ((sl + h) >> 2) * 128 + ((sl + h) & 3)));
                        }
                        const uint32_t c = min(s, 127u);
                        cv[8 * w + 4 * h + k] = c;
                        best = min(best, c);
                    }
                }
            }
        }
        any_pend = false;
        if (__builtin_expect(best < bsurv, 1)) {                // most wave iterations of a long level
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                // bytes >= bsurv -> 0xff, four at a time (all bytes and bsurv are <= 127: no borrow crosses a byte)
                const uint32_t p = cv[4 * w] | (cv[4 * w + 1] << 8) | (cv[4 * w + 2] << 16) | (cv[4 * w + 3] << 24);
                const uint32_t ge = ((p | 0x80808080u) - bound4) & 0x80808080u;
                pend[w] = p | ((ge >> 7) * 0xffu);
            }
            pend_base = base;
            any_pend = true;
        }
        }
        if (__builtin_expect(any_res, 0)) {                     // the previous iteration's candidates
            emit_res();
            any_res = false;
        }
    };
    if constexpr (PRUNE) {
        // The ids run kBktwRing tiles ahead of the tile loop, in a ring of registers: slot k holds the ids of the workgroup's tiles
        // k, k + D, k + 2 D, ...  The loop is unrolled D times, so that a slot is a fixed register and an iteration uses ids requested D
        // iterations ago.  That is the intent; what the compiler makes of it is less: it sizes the first body's wait as if one pair
        // were in flight, not D - 1, and zero-extends the narrow ids behind a full wait at the latch, so every D-th tile still ends
        // on the loads it has just issued (profiles/r15_bktw_loop.txt, with the rewrites that cured this and ran slower).  Every slot
        // is always loaded (no branch around a load): past the workgroup's last tile the ring re-reads that tile's ids (tlast), never
        // an id beyond the run; a workgroup without a tile loads nothing.
        if (first < last) {
            constexpr uint32_t D = kBktwRing;
            const uint32_t tlast = first + (last - 1u - first) / step * step;
            uint32_t rid[D], rid4[D];
#pragma unroll
            for (uint32_t k = 0; k < D; ++k) load_ids(min(first + k * step, tlast), rid[k], rid4[k]);   // (t + D step < 2^20: no wrap)
            uint32_t t = first;
            bool more = true;
            while (more) {
#pragma unroll
                for (uint32_t k = 0; k < D; ++k) {
                    const uint32_t id = rid[k], id4 = rid4[k];
                    load_ids(min(t + D * step, tlast), rid[k], rid4[k]);
                    step_tile(t, id, id4);
                    t += step;
                    if (t >= last) {
                        more = false;
                        break;
                    }
                }
            }
        }
    } else {
        for (uint32_t t = first; t < last; t += step) step_tile(t, 0u, 0u);
    }
    if (any_pend) {
        resolve();
        if (any_res) emit_res();
    }
    if (surv) {                                                 // (uniform) one global atomic per workgroup: the waves' counts meet in LDS
        uint32_t* cnt = reinterpret_cast<uint32_t*>(smem + C::HIST_OFF);
        __syncthreads();
        if (tid == 0) *cnt = 0;
        __syncthreads();
        const uint32_t tot = dpp_wave_incl_sum(nsurv);          // lane 63: the wave's count
        if ((tid & 63u) == 63u && tot) atomicAdd(cnt, tot);
        __syncthreads();
        if (tid == 0 && *cnt) atomicAdd(surv, (unsigned long long)*cnt);
    }
    if constexpr (PRUNE) {
        if (prune_cnt) {                                        // (uniform; profile option only) skipped, run, pruned, quarters: the same way
            uint32_t* cnt = reinterpret_cast<uint32_t*>(smem + C::HIST_OFF);
            const uint32_t niter = first < last ? (last - first + step - 1u) / step : 0u;   // the tile loop's trip count
            __syncthreads();
            if (tid < 4) cnt[tid] = 0;
            __syncthreads();
            if ((tid & 63u) == 0) {
                atomicAdd(cnt, nskip);
                atomicAdd(cnt + 1, niter - nskip);
                atomicAdd(cnt + 2, npruned);
                atomicAdd(cnt + 3, nquart);
            }
            __syncthreads();
            if (tid < 4 && cnt[tid]) atomicAdd(prune_cnt + tid, (unsigned long long)cnt[tid]);
        }
    }
}

template <int NSP, bool NT, bool CHUNK, bool PROBE>
__global__ __launch_bounds__(kWG, 8) void scan_i8_bkt_kernel(
    const ScanItem* __restrict__ items, const int8_t* __restrict__ qtables, QueryState* __restrict__ qstates,
    CandHeader* __restrict__ hdr, Cand* __restrict__ out, uint32_t cand_cap, uint32_t R,
    const uint8_t* __restrict__ bkt_sel, unsigned long long* __restrict__ surv) {
    scan_bkt_body<4, NSP, NT, CHUNK, PROBE, false>(items, qtables, qstates, hdr, out, cand_cap, R, bkt_sel, surv, nullptr);
}

// The wide form ("wide octaves"): the runs read wide tiles, bktw_sel = kBktwSelBytes per table (plane_choice_bktw).
template <int NSP, bool NT, bool CHUNK, bool PROBE>
__global__ __launch_bounds__(kWG, 8) void scan_i8_bktw_kernel(
    const ScanItem* __restrict__ items, const int8_t* __restrict__ qtables, QueryState* __restrict__ qstates,
    CandHeader* __restrict__ hdr, Cand* __restrict__ out, uint32_t cand_cap, uint32_t R,
    const uint8_t* __restrict__ bktw_sel, unsigned long long* __restrict__ surv) {
    scan_bkt_body<5, NSP, NT, CHUNK, PROBE, false>(items, qtables, qstates, hdr, out, cand_cap, R, bktw_sel, surv, nullptr);
}

// ... with the group test ("pruned groups"): a wave iteration in which no lane group can hold a survivor loads no
// plane and issues no pair lookup.  QUARTER (bkt_prune_lanes = 16): in an iteration that runs, a lane loads its planes only if
// some lane of its aligned 16-lane quarter keeps; the others present index 0 to the pair loop, which cannot make a survivor of
// them (every pair entry >= the sum of its rows' minima).  prune_cnt (profile option only, else null): wave iterations skipped,
// wave iterations run, lane groups pruned, quarters of run iterations without a load: one atomicAdd each per workgroup at exit.
// The second launch bound stays 8 like every streaming kernel's: it holds the compiler to 78 SGPRs, some 40 of the loop's uniform
// values then live in VGPR lanes, but with more than 80 SGPRs a SIMD takes fewer than 8 waves and a CU one workgroup of 1024, not
// two: the build with bound 2 (106 SGPRs, 10-12 spilled) ran the headline at 15.21 ms per step against 11.78
// (profiles/r14_bkt_tiles_lanes.txt).
template <int NSP, bool NT, bool CHUNK, bool PROBE, bool QUARTER>
__global__ __launch_bounds__(kWG, 8) void scan_i8_bktw_prune_kernel(
    const ScanItem* __restrict__ items, const int8_t* __restrict__ qtables, QueryState* __restrict__ qstates,
    CandHeader* __restrict__ hdr, Cand* __restrict__ out, uint32_t cand_cap, uint32_t R,
    const uint8_t* __restrict__ bktw_sel, unsigned long long* __restrict__ surv, unsigned long long* __restrict__ prune_cnt) {
    scan_bkt_body<5, NSP, NT, CHUNK, PROBE, true, QUARTER>(items, qtables, qstates, hdr, out, cand_cap, R, bktw_sel, surv, prune_cnt);
}


// The deferred byte of the 6-plane split form, once per int8 table: the j in 0..6 whose 256 pair entries
// q[2j][lo] + q[2j+1][hi] have the smallest sum = 16 x (the sum of the two 16-entry rows); ties: the highest j.
// The choice changes the survivor rate only, never a result.
__device__ __forceinline__ uint32_t plane_choice(const int8_t* __restrict__ qt) {
    const uint8_t* T = reinterpret_cast<const uint8_t*>(qt);
    uint32_t best = 0xffffffffu, bj = 6;
    for (uint32_t j = 0; j < 7; ++j) {
        uint32_t sum = 0;
        for (int i = 0; i < 32; ++i) sum += T[32 * j + i];
        if (sum <= best) { best = sum; bj = j; }
    }
    return bj;
}

// The two deferred bytes j1 < j2 of the 5-plane split form and its slack, once per int8 table: j1 | j2 << 4 | c << 8.
// With min P_j = min q[2j] + min q[2j+1] (the smallest entry of pair table j), score_j = the sum of the two rows
// - 16 min P_j = 1/16 of the sum of P_j[x] - min P_j over the 256 entries: what streaming byte j adds to the partial sum
// beyond what the slack already accounts for.  The two smallest scores are deferred (ties: the highest j, one pick after the
// other).  c = min(127, min P_j1 + min P_j2 + min P_7) is a lower bound of the deferred entries' sum for every code; a c
// above that sum would lose candidates, a poor choice of j only costs survivors.
__device__ __forceinline__ uint32_t plane_choice5(const int8_t* __restrict__ qt) {
    const uint8_t* T = reinterpret_cast<const uint8_t*>(qt);
    uint32_t score[7], minp[8];
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) {
        uint32_t sum = 0, m0 = 255u, m1 = 255u;
        for (int i = 0; i < 16; ++i) {
            const uint32_t a = T[32 * j + i], b = T[32 * j + 16 + i];
            sum += a + b;
            m0 = min(m0, a);
            m1 = min(m1, b);
        }
        minp[j] = m0 + m1;
        if (j < 7) score[j] = sum - 16u * minp[j];
    }
    uint32_t a = 6, b = 6;                                      // first and second pick
    uint32_t best = 0xffffffffu;
#pragma unroll
    for (uint32_t j = 0; j < 7; ++j)
        if (score[j] <= best) { best = score[j]; a = j; }
    best = 0xffffffffu;
#pragma unroll
    for (uint32_t j = 0; j < 7; ++j)
        if (j != a && score[j] <= best) { best = score[j]; b = j; }
    const uint32_t j1 = min(a, b), j2 = max(a, b);
    uint32_t mj1 = 0, mj2 = 0;                                  // (no dynamic index into minp[]: it stays in registers)
#pragma unroll
    for (uint32_t j = 0; j < 7; ++j) {
        mj1 = j == j1 ? minp[j] : mj1;
        mj2 = j == j2 ? minp[j] : mj2;
    }
    const uint32_t c = min(127u, mj1 + mj2 + minp[7]);
    return j1 | (j2 << 4) | (c << 8);
}

// The nibble form's choice, once per int8 table: the deferred sets of NS = 10, 9 and 8 streamed sub-quantizers and their
// slacks, kNibSelBytes bytes.  score_s = the sum of row s - 16 min T[s] = the sum of T[s][x] - min T[s] over the row: what
// streaming sub-quantizer s adds to the partial sum beyond what the slack already accounts for.  The smallest scores are
// deferred, one pick after the other (ties: the highest s), so the sets are nested: 6 picks for NS = 10, one more for 9, one
// more for 8.  c = min(127, the sum of min T[s] over the set) is a lower bound of the deferred entries' sum for every code;
// a c above that sum would lose candidates, a poor set only costs survivors.
__device__ __forceinline__ void plane_choice_nib(const int8_t* __restrict__ qt, uint8_t* __restrict__ out) {
    const uint8_t* T = reinterpret_cast<const uint8_t*>(qt);
    uint32_t score[16], mn[16];
#pragma unroll
    for (uint32_t s = 0; s < 16; ++s) {
        uint32_t sum = 0, m = 255u;
        for (int i = 0; i < 16; ++i) {
            const uint32_t a = T[16 * s + i];
            sum += a;
            m = min(m, a);
        }
        mn[s] = m;
        score[s] = sum - 16u * m;
    }
    uint32_t mask = 0, c = 0;
#pragma unroll
    for (uint32_t pick = 0; pick < 8; ++pick) {
        uint32_t best = 0xffffffffu, bs = 15, bm = 0;
#pragma unroll
        for (uint32_t s = 0; s < 16; ++s)
            if (!((mask >> s) & 1u) && score[s] <= best) { best = score[s]; bs = s; bm = mn[s]; }
        mask |= 1u << bs;
        c += bm;
        if (pick >= 5) {                                        // 6, 7, 8 deferred = NS 10, 9, 8
            uint8_t* o = out + 4u * (7u - pick);
            o[0] = (uint8_t)(mask & 0xffu);
            o[1] = (uint8_t)(mask >> 8);
            o[2] = (uint8_t)min(c, 127u);
            o[3] = 0;
        }
    }
}

// The bucket form's choice, once per int8 table: sub-quantizers 0-3 are free (the lane group's id), so the deferred sets are
// picked among 4..15 only, by plane_choice_nib's score and tie rule, nested: 5 picks for NSP = 7 paid planes, one more for
// 6, 5 and 4.  kBktSelBytes bytes: at 4 * (NSP - 4) the set as a 16-bit mask (low byte first), c = min(127, the sum of min T[s]
// over the set), 0.  A c above the deferred entries' sum would lose candidates, a poor set only costs survivors.
template <uint32_t FIRST>
__device__ __forceinline__ void plane_choice_bkt_from(const int8_t* __restrict__ qt, uint8_t* __restrict__ out) {
    const uint8_t* T = reinterpret_cast<const uint8_t*>(qt);
    uint32_t score[16], mn[16];
#pragma unroll
    for (uint32_t s = FIRST; s < 16; ++s) {
        uint32_t sum = 0, m = 255u;
        for (int i = 0; i < 16; ++i) {
            const uint32_t a = T[16 * s + i];
            sum += a;
            m = min(m, a);
        }
        mn[s] = m;
        score[s] = sum - 16u * m;
    }
    uint32_t mask = 0, c = 0;
#pragma unroll
    for (uint32_t pick = 0; pick < 8; ++pick) {
        uint32_t best = 0xffffffffu, bs = 15, bm = 0;
#pragma unroll
        for (uint32_t s = FIRST; s < 16; ++s)
            if (!((mask >> s) & 1u) && score[s] <= best) { best = score[s]; bs = s; bm = mn[s]; }
        mask |= 1u << bs;
        c += bm;
        if (pick >= 4) {                                        // 5, 6, 7, 8 deferred = NSP 7, 6, 5, 4 (FIRST = 5: NSP 6, 5, 4, 3)
            uint8_t* o = out + 4u * (7u - pick);
            o[0] = (uint8_t)(mask & 0xffu);
            o[1] = (uint8_t)(mask >> 8);
            o[2] = (uint8_t)min(c, 127u);
            o[3] = 0;
        }
    }
}
__device__ __forceinline__ void plane_choice_bkt(const int8_t* __restrict__ qt, uint8_t* __restrict__ out) {
    plane_choice_bkt_from<4>(qt, out);
}
// The wide form's choice: sub-quantizers 0-4 are free, so the same picks run among 5..15: 5 picks for NSP = 6 paid planes, one more
// for 5, 4 and 3.  kBktwSelBytes bytes: at 4 * (NSP - 3) the mask, c, 0.
__device__ __forceinline__ void plane_choice_bktw(const int8_t* __restrict__ qt, uint8_t* __restrict__ out) {
    static_assert(kBktwSelBytes == kBktSelBytes, "the same four records");
    plane_choice_bkt_from<5>(qt, out);
}

// plane_sel (6-plane form, 1 byte per table), plane_sel5 (5-plane form, 2 bytes per table), nib_sel (nibble form, kNibSelBytes
// per table) and bkt_sel (bucket form, kBktSelBytes per table): each may be null
__global__ __launch_bounds__(256) void plane_choice_kernel(const int8_t* __restrict__ qtables, int ntables, uint8_t* __restrict__ plane_sel,
                                                           uint8_t* __restrict__ plane_sel5, uint8_t* __restrict__ nib_sel,
                                                           uint8_t* __restrict__ bkt_sel, uint8_t* __restrict__ bktw_sel) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= ntables) return;
    if (plane_sel) plane_sel[t] = (uint8_t)plane_choice(qtables + (size_t)t * 256);
    if (plane_sel5) {
        const uint32_t c5 = plane_choice5(qtables + (size_t)t * 256);
        plane_sel5[2 * (size_t)t] = (uint8_t)(c5 & 0xffu);
        plane_sel5[2 * (size_t)t + 1] = (uint8_t)(c5 >> 8);
    }
    if (nib_sel) plane_choice_nib(qtables + (size_t)t * 256, nib_sel + (size_t)t * kNibSelBytes);
    if (bkt_sel) plane_choice_bkt(qtables + (size_t)t * 256, bkt_sel + (size_t)t * kBktSelBytes);
    if (bktw_sel) plane_choice_bktw(qtables + (size_t)t * 256, bktw_sel + (size_t)t * kBktwSelBytes);
}

void launch_plane_choice(const int8_t* d_qtables, int ntables, uint8_t* d_plane_sel, hipStream_t stream, uint8_t* d_plane_sel5,
                         uint8_t* d_nib_sel, uint8_t* d_bkt_sel, uint8_t* d_bktw_sel) {
    if (ntables <= 0 || (!d_plane_sel && !d_plane_sel5 && !d_nib_sel && !d_bkt_sel && !d_bktw_sel)) return;
    hipLaunchKernelGGL(plane_choice_kernel, dim3((ntables + 255) / 256), dim3(256), 0, stream, d_qtables, ntables, d_plane_sel,
                       d_plane_sel5, d_nib_sel, d_bkt_sel, d_bktw_sel);
}

// The byte-plane copy of a partition (kSplitTile layout): one thread per 16 codes of a tile, plane b's 16 bytes = byte b
// of the 16 codes.  Reads the row-major codes once, writes 7/8 of them; run once per partition by qadc_index_finalize.
__global__ __launch_bounds__(256) void split_copy_kernel(const uint8_t* __restrict__ codes, uint32_t n, uint8_t* __restrict__ copy,
                                                         uint64_t nthreads) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= nthreads) return;
    const uint64_t tile = g / (kSplitTile / 16), lane = g % (kSplitTile / 16);
    const uint64_t c0 = tile * kSplitTile + lane * 16;
    uint32_t o[kSplitBytes][4] = {};
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        uint2 v = make_uint2(0u, 0u);
        if (c0 + c < n) v = *reinterpret_cast<const uint2*>(codes + (c0 + c) * 8);
#pragma unroll
        for (int b = 0; b < (int)kSplitBytes; ++b) {
            const uint32_t byte = ((b < 4 ? v.x : v.y) >> (8 * (b & 3))) & 0xffu;
            o[b][c >> 2] |= byte << (8 * (c & 3));
        }
    }
#pragma unroll
    for (int b = 0; b < (int)kSplitBytes; ++b)
        *reinterpret_cast<uint4*>(copy + tile * kSplitBytes * kSplitTile + (uint64_t)b * kSplitTile + lane * 16) =
            make_uint4(o[b][0], o[b][1], o[b][2], o[b][3]);
}

void launch_split_copy(const uint8_t* d_codes, uint32_t n, uint8_t* d_copy, hipStream_t stream) {
    const uint64_t nthreads = ((uint64_t)n + kSplitTile - 1) / kSplitTile * (kSplitTile / 16);
    if (!nthreads) return;
    hipLaunchKernelGGL(split_copy_kernel, dim3((unsigned)((nthreads + 255) / 256)), dim3(256), 0, stream, d_codes, n, d_copy, nthreads);
}

// The nibble-plane copy of a partition (kNibTileBytes per tile): one thread per 16 codes of a tile; plane s gets the lane's two
// dwords, byte k of dword w = sub-quantizer s of code 8 w + k (low nibble) and of code 8 w + 4 + k (high nibble).  Reads the
// row-major codes once and writes as many bytes; run once per partition by qadc_index_finalize.
__global__ __launch_bounds__(256) void nib_copy_kernel(const uint8_t* __restrict__ codes, uint32_t n, uint8_t* __restrict__ copy,
                                                       uint64_t nthreads) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= nthreads) return;
    const uint64_t tile = g / (kSplitTile / 16), lane = g % (kSplitTile / 16);
    const uint64_t c0 = tile * kSplitTile + lane * 16;
    uint32_t o[16][2] = {};
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        uint2 v = make_uint2(0u, 0u);
        if (c0 + c < n) v = *reinterpret_cast<const uint2*>(codes + (c0 + c) * 8);
        const int sh = 8 * (c & 3) + 4 * ((c >> 2) & 1);
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const uint32_t nibble = ((s < 8 ? v.x : v.y) >> (4 * (s & 7))) & 15u;
            o[s][c >> 3] |= nibble << sh;
        }
    }
#pragma unroll
    for (int s = 0; s < 16; ++s)
        *reinterpret_cast<uint2*>(copy + tile * kNibTileBytes + (uint64_t)s * (kSplitTile / 2) + lane * 8) = make_uint2(o[s][0], o[s][1]);
}

void launch_nib_copy(const uint8_t* d_codes, uint32_t n, uint8_t* d_copy, hipStream_t stream) {
    const uint64_t nthreads = ((uint64_t)n + kSplitTile - 1) / kSplitTile * (kSplitTile / 16);
    if (!nthreads) return;
    hipLaunchKernelGGL(nib_copy_kernel, dim3((unsigned)((nthreads + 255) / 256)), dim3(256), 0, stream, d_codes, n, d_copy, nthreads);
}

// ---- the bucket copy of a partition (host/level_plan.hpp has the layout), block by block; run once per partition by
// qadc_index_finalize, not timed.  The scatter is UNSTABLE: a code's slot inside its bucket is the order in which its atomicAdd on
// the bucket's cursor lands, so two builds of the same partition may order a bucket differently.  No result depends on that order.
// Key histogram of one block: codes = the block's first code, n = its codes; hist[nkeys], zeroed by the caller.  nkeys = kBktKeys
// (narrow block: code bytes 0 and 1) or kBktwKeys (wide octave: and the low nibble of byte 2): key = the code's low bits.
__global__ __launch_bounds__(256) void bkt_hist_kernel(const uint8_t* __restrict__ codes, uint32_t n, uint32_t* __restrict__ hist,
                                                       uint32_t nkeys) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        atomicAdd(&hist[*reinterpret_cast<const uint32_t*>(codes + i * 8) & (nkeys - 1u)], 1u);
}

// Exclusive scan of the bucket sizes, each padded to a multiple of 16 slots: off[key] = first slot of the bucket in its block.
// hist comes back zeroed (the scatter's cursors).  info[0] = the block's slots, padded to whole tiles; info[1] = its last real slot.
// One workgroup of 1024 threads, kpt = nkeys / 1024 consecutive keys each (64, or 1024 for a wide octave).
__global__ __launch_bounds__(1024) void bkt_scan_kernel(uint32_t* __restrict__ hist, uint32_t* __restrict__ off, uint32_t* __restrict__ info,
                                                        uint32_t kpt) {
    static_assert(kBktKeys % 1024 == 0 && kBktwKeys % 1024 == 0, "whole keys per thread");
    __shared__ uint32_t wave_sum[16];
    __shared__ uint32_t last_real;
    const uint32_t t = threadIdx.x;
    if (t == 0) last_real = 0;
    uint32_t mine = 0;
    for (uint32_t k = 0; k < kpt; ++k) mine += (hist[kpt * t + k] + 15u) & ~15u;
    const uint32_t incl = dpp_wave_incl_sum(mine);
    if ((t & 63u) == 63u) wave_sum[t >> 6] = incl;
    __syncthreads();
    uint32_t run = incl - mine;
    for (uint32_t w = 0; w < (t >> 6); ++w) run += wave_sum[w];
    uint32_t end_real = 0;
    for (uint32_t k = 0; k < kpt; ++k) {
        const uint32_t c = hist[kpt * t + k];
        off[kpt * t + k] = run;
        if (c) end_real = run + c;
        run += (c + 15u) & ~15u;
        hist[kpt * t + k] = 0;
    }
    if (end_real) atomicMax(&last_real, end_real - 1u);
    __syncthreads();
    if (t == 1023) {
        info[0] = (run + kSplitTile - 1) / kSplitTile * kSplitTile;
        info[1] = last_real;
    }
}

// Scatter of one block: code i of the block goes to slot off[key] + (its turn at the bucket's cursor) of the block's first tile
// `side` of the side array, with its position pos_first + i in the partition.  The side array's perm words are kBktPad beforehand.
__global__ __launch_bounds__(256) void bkt_scatter_kernel(const uint8_t* __restrict__ codes, uint32_t n, uint32_t pos_first,
                                                          const uint32_t* __restrict__ off, uint32_t* __restrict__ cursor,
                                                          uint8_t* __restrict__ side, uint32_t nkeys) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint2 v = *reinterpret_cast<const uint2*>(codes + i * 8);
        const uint32_t key = v.x & (nkeys - 1u);
        const uint32_t slot = off[key] + atomicAdd(&cursor[key], 1u);
        uint8_t* tile = side + (uint64_t)(slot / kSplitTile) * kBktSideBytes;
        *reinterpret_cast<uint2*>(tile + (uint64_t)(slot % kSplitTile) * 8) = v;
        *reinterpret_cast<uint32_t*>(tile + kBktPermOff + (uint64_t)(slot % kSplitTile) * 4) = pos_first + (uint32_t)i;
    }
}

// Padding and planes of one block, one thread per 16-slot group: the padding slots of the group (perm == kBktPad; they follow the
// bucket's real slots) get the code of the group's last real slot, a group without one (the block's tail) the code of the block's
// last real slot; then the group's 12 nibble planes (nib_copy_kernel's in-plane layout) and its id are written.  WIDE: the 11
// planes of sub-quantizers 5-15, the uint16 id and the byte of sub-quantizer 4 of a wide tile.
template <bool WIDE>
__global__ __launch_bounds__(256) void bkt_fill_kernel(uint8_t* __restrict__ tiles, uint8_t* __restrict__ side, uint32_t slots,
                                                       uint32_t last_real) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= slots / 16) return;
    const uint64_t tile = g / (kSplitTile / 16), lane = g % (kSplitTile / 16);
    uint8_t* st = side + tile * kBktSideBytes;
    uint2 v[16];
    int last = -1;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        v[c] = *reinterpret_cast<const uint2*>(st + (lane * 16 + c) * 8);
        if (*reinterpret_cast<const uint32_t*>(st + kBktPermOff + (lane * 16 + c) * 4) != kBktPad) last = c;
    }
    uint2 fillv = *reinterpret_cast<const uint2*>(side + (uint64_t)(last_real / kSplitTile) * kBktSideBytes +
                                                  (uint64_t)(last_real % kSplitTile) * 8);
#pragma unroll
    for (int c = 0; c < 16; ++c) fillv = c == last ? v[c] : fillv;
    constexpr int kFirst = WIDE ? 5 : 4, kPl = WIDE ? (int)kBktwPlanes : (int)kBktPlanes;
    uint32_t o[kPl][2] = {};
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        if (c > last) {
            v[c] = fillv;
            *reinterpret_cast<uint2*>(st + (lane * 16 + c) * 8) = fillv;
        }
        const int sh = 8 * (c & 3) + 4 * ((c >> 2) & 1);
#pragma unroll
        for (int s = kFirst; s < 16; ++s) {
            const uint32_t nibble = ((s < 8 ? v[c].x : v[c].y) >> (4 * (s & 7))) & 15u;
            o[s - kFirst][c >> 3] |= nibble << sh;
        }
    }
    uint8_t* tt = tiles + tile * (WIDE ? kBktwTileBytes : kBktTileBytes);
#pragma unroll
    for (int s = 0; s < kPl; ++s)
        *reinterpret_cast<uint2*>(tt + (uint64_t)s * (kSplitTile / 2) + lane * 8) = make_uint2(o[s][0], o[s][1]);
    *reinterpret_cast<uint16_t*>(tt + (WIDE ? kBktwIdOff : kBktIdOff) + lane * 2) = (uint16_t)(v[0].x & 0xffffu);
    if (WIDE) tt[kBktwId4Off + lane] = (uint8_t)((v[0].x >> 16) & 15u);
}

void launch_bkt_hist_scan(const uint8_t* d_codes, uint32_t n, uint32_t* d_hist, uint32_t* d_off, uint32_t* d_info, hipStream_t stream,
                          bool wide) {
    if (!n) return;
    const uint32_t nkeys = wide ? kBktwKeys : kBktKeys;
    const unsigned wgs = (unsigned)std::min<uint64_t>(((uint64_t)n + 255) / 256, 8192);
    hipLaunchKernelGGL(bkt_hist_kernel, dim3(wgs), dim3(256), 0, stream, d_codes, n, d_hist, nkeys);
    hipLaunchKernelGGL(bkt_scan_kernel, dim3(1), dim3(1024), 0, stream, d_hist, d_off, d_info, nkeys / 1024u);
}

void launch_bkt_scatter_fill(const uint8_t* d_codes, uint32_t n, uint32_t pos_first, const uint32_t* d_off, uint32_t* d_cursor,
                             uint8_t* d_tiles, uint8_t* d_side, uint32_t slots, uint32_t last_real, hipStream_t stream, bool wide) {
    if (!n || !slots) return;
    const unsigned wgs = (unsigned)std::min<uint64_t>(((uint64_t)n + 255) / 256, 8192);
    hipLaunchKernelGGL(bkt_scatter_kernel, dim3(wgs), dim3(256), 0, stream, d_codes, n, pos_first, d_off, d_cursor, d_side,
                       wide ? kBktwKeys : kBktKeys);
    if (wide)
        hipLaunchKernelGGL(bkt_fill_kernel<true>, dim3((slots / 16 + 255) / 256), dim3(256), 0, stream, d_tiles, d_side, slots, last_real);
    else
        hipLaunchKernelGGL(bkt_fill_kernel<false>, dim3((slots / 16 + 255) / 256), dim3(256), 0, stream, d_tiles, d_side, slots, last_real);
}

// ---------------------------------------------------------------------------------------------
// Multi-query streaming scan: ONE pass over the codes serves up to 8 queries.
//
// Once the queries of a batch share the codes through L2 (sibling-major launch above), scan_i8_kernel is bound
// by the LDS lookup pipe: one ds_read_u8 per (code byte, query) = 2 LDS cycles per 64 lookups, and 3/4 of every
// bank access is thrown away.  Here a lookup returns the entries of EIGHT queries at once:
//
//   LDS image: for sub-quantizer t and centroid x, row (t, x) = { T_q[t][x] as u16 : q = 0..7 } = 16 bytes at
//              t*256 + x*16.  One ds_read_b128 per code nibble = 4 LDS cycles per 64 lanes x 8 queries,
//              i.e. 8 LDS cycles per (64 codes, query) against 16.
//   No replication: a 16-lane ds_read_b128 group conflicts only when two lanes want DIFFERENT rows in the same
//   banks; the 16 rows of a table tile the 64 banks exactly once, and lanes that want the same row are one
//   broadcast.  Conflict-free for any code data, in 4 KiB (16x4) / 8 KiB (32x4) of LDS instead of 64 / 128 KiB.
//   Sums: the 16-bit fields never overflow (<= 32 x 127), so a row is added as TWO 64-bit integers
//   (v_lshl_add_u64: 4 queries per instruction, half the instructions of v_pk_add_u16), no widening, no
//   per-query loop.
//   Test: adding (0x8000 - bound) to every field sets the field's top bit iff sum >= bound (no carry between
//   fields: <= 4064 + 32768); the results are AND-ed over the U x CPL codes of an iteration and tested with ONE
//   branch; the rare path emits per query exactly as scan_i8_kernel does.
//
// Exactness is untouched: the same integer sums, the same prefix bound per query, the same candidates.
// ---------------------------------------------------------------------------------------------
constexpr int kMQ = 8;          // queries per pass
constexpr int kMQWG = 256;      // threads per workgroup

typedef uint16_t u16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));
typedef const __attribute__((address_space(3))) u64x2* lds_row_t;

// wave-level prefix bound (no LDS, no barrier): lane l owns value bins 2l and 2l+1
__device__ __forceinline__ uint32_t prefix_bound_wave(const QueryState* qs, int level, uint32_t R, uint32_t lane) {
    uint32_t c0 = 0, c1 = 0;
    for (int l = 0; l < level; ++l) {
        const uint2 h = *reinterpret_cast<const uint2*>(&qs->hist[l * 128 + 2 * lane]);
        c0 += h.x;
        c1 += h.y;
    }
    const uint32_t incl = dpp_wave_incl_sum(c0 + c1);
    const uint32_t excl = incl - (c0 + c1);
    const uint64_t reached = __builtin_amdgcn_ballot_w64(incl >= R);
    if (reached == 0) return 127u;
    const uint32_t b = excl + c0 >= R ? 2 * lane : 2 * lane + 1;   // (meaningful in the first lane that reaches R)
    return min((uint32_t)__builtin_amdgcn_readlane((int)b, (int)__builtin_ctzll(reached)), 127u);
}

// (byte K of d) & mask in ONE VALU instruction (sub-dword operand select); the compiler finds this form for only a
// quarter of the lookups by itself and spends a shift + and on the others
template <int K>
__device__ __forceinline__ uint32_t byte_and(uint32_t d, uint32_t mask) {
    uint32_t r;
    // (a plain v_and_b32 for byte 0 — full issue rate on gfx950, every SDWA form half — was tried in round 5: nothing at the IVF
    //  shapes, +0.6 % on the flat batched step, profiles/r05_byte0_and_ab.txt)
    if (K == 0) asm("v_and_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_0" : "=v"(r) : "v"(mask), "v"(d));
    if (K == 1) asm("v_and_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_1" : "=v"(r) : "v"(mask), "v"(d));
    if (K == 2) asm("v_and_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_2" : "=v"(r) : "v"(mask), "v"(d));
    if (K == 3) asm("v_and_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_3" : "=v"(r) : "v"(mask), "v"(d));
    return r;
}

typedef uint64_t u64x1 __attribute__((ext_vector_type(1)));
template <int NQ> struct MqRow;
template <> struct MqRow<8> { typedef u64x2 type; };          // 8 queries: 16-byte rows, ds_read_b128
template <> struct MqRow<4> { typedef u64x1 type; };          // 4 queries:  8-byte rows, ds_read_b64 (half the LDS cycles)

// One group's pass with NQ = 8 or 4 query seats.  A group whose live seats fit 4 (the remainder groups of the IVF second
// phase: seats are filled from 0 upward) takes the 4-seat form: the same lookups return 8 bytes instead of 16, i.e. 4 LDS
// cycles per (64 codes, nibble pair) instead of 8, and half the adds.
template <int M, int U, int NQ, bool PIPE>
__device__ __forceinline__ void scan_mq_body(const ScanItem* __restrict__ its, const ScanItem& it, int nq, uint32_t bx, uint32_t G,
                                             const int8_t* __restrict__ qtables, QueryState* __restrict__ qstates,
                                             CandHeader* __restrict__ hdr, Cand* __restrict__ out, uint32_t cand_cap, uint32_t R) {
    constexpr int CS = M / 2, DW = M / 8, CPL = 16 / CS;
    constexpr int ROWB = 2 * NQ, NW = NQ / 4;                    // bytes per row, u64 words per row
    typedef typename MqRow<NQ>::type row_t;
    typedef const __attribute__((address_space(3))) row_t* lds_rowq_t;
    constexpr int TAB = M * 256;                                 // bytes reserved for the row image; then u32 bound[8]
    uint32_t* lbound = reinterpret_cast<uint32_t*>(smem + TAB);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;

    // ---- row image: thread -> (t, x); the queries' entries widened to u16; absent queries read as 0 ----
    for (int e = tid; e < M * 16; e += kMQWG) {
        uint16_t row[NQ];
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            uint16_t v = 0;
            if (j < nq && its[j].n != 0) v = (uint16_t)(uint8_t)qtables[(uint64_t)its[j].table * (M * 16) + e];   // (n == 0: empty seat)
            row[j] = v;
        }
        uint64_t* dst = reinterpret_cast<uint64_t*>(smem + e * ROWB);   // little-endian: query j = field j&3 of u64 j>>2
#pragma unroll
        for (int w = 0; w < NW; ++w)
            dst[w] = (uint64_t)row[4 * w] | ((uint64_t)row[4 * w + 1] << 16) | ((uint64_t)row[4 * w + 2] << 32) | ((uint64_t)row[4 * w + 3] << 48);
    }
    // ---- bounds: wave w computes queries w, w+4 (absent queries: 0 = nothing qualifies) ----
    for (int j = (int)wave; j < NQ; j += kMQWG / 64) {
        uint32_t b = 0;
        if (j < nq && its[j].n != 0) b = prefix_bound_wave(qstates + its[j].query, its[j].order >> 16, R, lane);
        if (lane == 0) lbound[j] = b;
    }
    __syncthreads();
    uint32_t bq[NQ];
    uint64_t bias[NW];                                           // (0x8000 - bound) in every 16-bit field
#pragma unroll
    for (int w = 0; w < NW; ++w) bias[w] = 0;
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
        bq[j] = __builtin_amdgcn_readfirstlane(lbound[j]);
        bias[j >> 2] |= (uint64_t)(0x8000u - bq[j]) << (16 * (j & 3));
    }
    constexpr uint64_t kTop = 0x8000800080008000ull;

    typedef const __attribute__((address_space(1))) u32x4_t* gvec_t;
    const gvec_t src = (gvec_t)(uintptr_t)it.codes;
    const uint32_t n = it.n;
    const uint32_t nvec = (n + CPL - 1) / CPL;
    const uint32_t ntiles = (nvec + kMQWG - 1) / kMQWG;

    // row offset = x * ROWB.  16-byte rows: the high nibble of byte k is (byte k) & 0xf0, the low one the same of d << 4;
    // 8-byte rows: (d >> 1) & 0x78 and (d << 3) & 0x78 (the bits that cross a byte boundary fall outside the mask)
    constexpr uint32_t nib_mask = NQ == 8 ? 0xf0u : 0x78u;
    // sums of the NQ queries for one code (DW dwords at d)
    auto code_sums = [&](const uint32_t* d) -> row_t {
        row_t a = {};
#pragma unroll
        for (int w = 0; w < DW; ++w) {
            const uint32_t dl = NQ == 8 ? d[w] << 4 : d[w] << 3;
            const uint32_t dh = NQ == 8 ? d[w] : d[w] >> 1;
#define QADC_MQ_BYTE(k)                                                                                        \
            {                                                                                                  \
                /* code byte b = 4w + k: sub-quantizer 2b takes the low nibble, 2b+1 the high one */           \
                const int t0 = 2 * (4 * w + (k));                                                              \
                const uint32_t xl = byte_and<(k)>(dl, nib_mask), xh = byte_and<(k)>(dh, nib_mask);             \
                a += *reinterpret_cast<lds_rowq_t>(static_cast<uintptr_t>(xl + t0 * (16 * ROWB)));             \
                a += *reinterpret_cast<lds_rowq_t>(static_cast<uintptr_t>(xh + (t0 + 1) * (16 * ROWB)));       \
            }
            QADC_MQ_BYTE(0) QADC_MQ_BYTE(1) QADC_MQ_BYTE(2) QADC_MQ_BYTE(3)
#undef QADC_MQ_BYTE
        }
        return a;
    };

    auto run = [&](uint32_t t0, auto full) {
        u32x4_t v[U];
        uint32_t e[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t t = t0 + u * G;
            e[u] = t * kMQWG + tid;
            if (decltype(full)::value) {
                v[u] = src[e[u]];
            } else {
                v[u] = u32x4_t{0, 0, 0, 0};
                if (t < ntiles && e[u] < nvec) v[u] = src[e[u]];
                else e[u] = 0xffffffffu;
            }
        }
        row_t sums[U * CPL];
        uint64_t all[NW];                                        // stays kTop while no field is below its bound
#pragma unroll
        for (int w = 0; w < NW; ++w) all[w] = kTop;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t d[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
            for (int c = 0; c < CPL; ++c) {
                const row_t a = code_sums(d + c * DW);
                sums[u * CPL + c] = a;
                const bool live = decltype(full)::value || (e[u] != 0xffffffffu && e[u] * CPL + c < n);
#pragma unroll
                for (int w = 0; w < NW; ++w) {
                    const uint64_t t = a[w] + bias[w];           // field top bit: sum >= bound
                    all[w] &= live ? t : kTop;
                }
            }
        }
        uint64_t allw = all[0];
#pragma unroll
        for (int w = 1; w < NW; ++w) allw &= all[w];
        if (__builtin_expect((allw & kTop) != kTop, 0)) {        // rare
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int c = 0; c < CPL; ++c) {
                    if (!decltype(full)::value && !(e[u] != 0xffffffffu && e[u] * CPL + c < n)) continue;
#pragma unroll
                    for (int j = 0; j < NQ; ++j) {
                        const uint32_t sj = (uint32_t)(sums[u * CPL + c][j >> 2] >> (16 * (j & 3))) & 0xffffu;
                        if (sj < bq[j]) {
                            const ScanItem* ij = its + j;
                            emit_candidate(qstates + ij->query, hdr, out + (uint64_t)ij->query * cand_cap, cand_cap,
                                           it.labels, it.key_base, ij->order, it.dup_pos, it.dup_reps,
                                           it.pos0 + e[u] * CPL + c, sj);
                        }
                    }
                }
        }
    };
    using full_t = std::integral_constant<bool, true>;
    using part_t = std::integral_constant<bool, false>;
    const uint32_t tiles_full = (n / CPL) / kMQWG;           // tiles whose every lane holds CPL complete codes
    uint32_t t0 = bx;
    if constexpr (PIPE) {
        // software pipeline over the full tiles (the IVF second phase: runs of a few 10^4 codes that come from HBM, one or two
        // groups per partition): the next iteration's loads are issued before the current tiles are looked up, so a wave
        // keeps loads in flight while it works the LDS pipe.  Without it a wave holds 2 KB in flight for ~3 us and then
        // nothing while it computes: 28 waves x 2 KB per CU bound the launch below the LDS roof (C3 shape: 2.9 TB/s of reads)
        auto consume = [&](const u32x4_t (&v)[U], uint32_t tt) {
            row_t sums[U * CPL];
            uint64_t all[NW];
#pragma unroll
            for (int w = 0; w < NW; ++w) all[w] = kTop;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint32_t d[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
                for (int c = 0; c < CPL; ++c) {
                    const row_t a = code_sums(d + c * DW);
                    sums[u * CPL + c] = a;
#pragma unroll
                    for (int w = 0; w < NW; ++w) all[w] &= a[w] + bias[w];
                }
            }
            uint64_t allw = all[0];
#pragma unroll
            for (int w = 1; w < NW; ++w) allw &= all[w];
            if (__builtin_expect((allw & kTop) != kTop, 0)) {        // rare
#pragma unroll
                for (int u = 0; u < U; ++u)
#pragma unroll
                    for (int c = 0; c < CPL; ++c)
#pragma unroll
                        for (int j = 0; j < NQ; ++j) {
                            const uint32_t sj = (uint32_t)(sums[u * CPL + c][j >> 2] >> (16 * (j & 3))) & 0xffffu;
                            if (sj < bq[j]) {
                                const ScanItem* ij = its + j;
                                emit_candidate(qstates + ij->query, hdr, out + (uint64_t)ij->query * cand_cap, cand_cap,
                                               it.labels, it.key_base, ij->order, it.dup_pos, it.dup_reps,
                                               it.pos0 + ((tt + u * G) * kMQWG + tid) * CPL + c, sj);
                            }
                        }
            }
        };
        if (t0 + (U - 1) * G < tiles_full) {
            u32x4_t v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = src[(t0 + u * G) * kMQWG + tid];
            for (;;) {
                const uint32_t tn = t0 + G * U;
                const bool more_full = tn + (U - 1) * G < tiles_full;
                u32x4_t nv[U];
                if (more_full) {
#pragma unroll
                    for (int u = 0; u < U; ++u) nv[u] = src[(tn + u * G) * kMQWG + tid];
                }
                consume(v, t0);
                t0 = tn;
                if (!more_full) break;
#pragma unroll
                for (int u = 0; u < U; ++u) v[u] = nv[u];
            }
        }
    } else {
        for (; t0 + (U - 1) * G < tiles_full; t0 += G * U) run(t0, full_t());
    }
    for (; t0 < ntiles; t0 += G * U) run(t0, part_t());
}

// Round 5: two more seat counts for the IVF second phase (scan_mq_body_x).  A group with 1-2 live seats reads 4-byte rows
// (one LDS cycle per 64 lookups instead of two, v_add_u32 adds at full issue rate), one with 5-6 reads 12 of a 16-byte row
// (ds_read_b64 + ds_read_b32: three LDS cycles instead of four, three dword adds instead of two 64-bit ones).  Rows are kept
// as dwords of two u16 fields; everything else — bounds, bias test, rare emit path, software pipeline — as in scan_mq_body.
template <int M, int U, int NQ>
__device__ __forceinline__ void scan_mq_body_x(const ScanItem* __restrict__ its, const ScanItem& it, int nq, uint32_t bx, uint32_t G,
                                               const int8_t* __restrict__ qtables, QueryState* __restrict__ qstates,
                                               CandHeader* __restrict__ hdr, Cand* __restrict__ out, uint32_t cand_cap, uint32_t R) {
    static_assert(NQ == 2 || NQ == 6, "seat counts of this body");
    constexpr int CS = M / 2, DW = M / 8, CPL = 16 / CS;
    constexpr int ROWB = NQ == 2 ? 4 : 16, ND = NQ / 2;          // bytes per row, dwords used per row
    constexpr int TAB = M * 256;
    typedef const __attribute__((address_space(3))) uint32_t* lds_u32_t;
    typedef const __attribute__((address_space(3))) uint64_t* lds_u64_t;
    uint32_t* lbound = reinterpret_cast<uint32_t*>(smem + TAB);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    for (int e = tid; e < M * 16; e += kMQWG) {
        uint32_t dwv[ND];
#pragma unroll
        for (int w = 0; w < ND; ++w) {
            uint32_t lo = 0, hi = 0;
            if (2 * w < nq && its[2 * w].n != 0) lo = (uint8_t)qtables[(uint64_t)its[2 * w].table * (M * 16) + e];
            if (2 * w + 1 < nq && its[2 * w + 1].n != 0) hi = (uint8_t)qtables[(uint64_t)its[2 * w + 1].table * (M * 16) + e];
            dwv[w] = lo | (hi << 16);
        }
        uint32_t* dst = reinterpret_cast<uint32_t*>(smem + e * ROWB);
#pragma unroll
        for (int w = 0; w < ND; ++w) dst[w] = dwv[w];
    }
    for (int j = (int)wave; j < NQ; j += kMQWG / 64) {
        uint32_t b = 0;
        if (j < nq && its[j].n != 0) b = prefix_bound_wave(qstates + its[j].query, its[j].order >> 16, R, lane);
        if (lane == 0) lbound[j] = b;
    }
    __syncthreads();
    uint32_t bq[NQ], bias[ND];
#pragma unroll
    for (int j = 0; j < NQ; ++j) bq[j] = __builtin_amdgcn_readfirstlane(lbound[j]);
#pragma unroll
    for (int w = 0; w < ND; ++w) bias[w] = (0x8000u - bq[2 * w]) | ((0x8000u - bq[2 * w + 1]) << 16);
    constexpr uint32_t kTop = 0x80008000u;

    typedef const __attribute__((address_space(1))) u32x4_t* gvec_t;
    const gvec_t src = (gvec_t)(uintptr_t)it.codes;
    const uint32_t n = it.n;
    const uint32_t nvec = (n + CPL - 1) / CPL;
    const uint32_t ntiles = (nvec + kMQWG - 1) / kMQWG;
    constexpr uint32_t nib_mask = NQ == 2 ? 0x3cu : 0xf0u;
    struct Row { uint32_t d[ND]; };
    auto code_sums = [&](const uint32_t* d) -> Row {
        Row a;
#pragma unroll
        for (int w = 0; w < ND; ++w) a.d[w] = 0;
#pragma unroll
        for (int w = 0; w < DW; ++w) {
            const uint32_t dl = NQ == 2 ? d[w] << 2 : d[w] << 4;
            const uint32_t dh = NQ == 2 ? d[w] >> 2 : d[w];
#define QADC_MQX_READ(addr)                                                                                    \
            {                                                                                                  \
                if (NQ == 2) {                                                                                 \
                    a.d[0] += *reinterpret_cast<lds_u32_t>(static_cast<uintptr_t>(addr));                      \
                } else {                                                                                       \
                    const uint64_t r01 = *reinterpret_cast<lds_u64_t>(static_cast<uintptr_t>(addr));           \
                    const uint32_t r2 = *reinterpret_cast<lds_u32_t>(static_cast<uintptr_t>((addr) + 8));      \
                    a.d[0] += (uint32_t)r01;                                                                   \
                    a.d[1] += (uint32_t)(r01 >> 32);                                                           \
                    a.d[ND - 1] += r2;                                                                         \
                }                                                                                              \
            }
#define QADC_MQX_BYTE(k)                                                                                       \
            {                                                                                                  \
                const int t0 = 2 * (4 * w + (k));                                                              \
                const uint32_t xl = byte_and<(k)>(dl, nib_mask), xh = byte_and<(k)>(dh, nib_mask);             \
                QADC_MQX_READ(xl + t0 * (16 * ROWB))                                                           \
                QADC_MQX_READ(xh + (t0 + 1) * (16 * ROWB))                                                     \
            }
            QADC_MQX_BYTE(0) QADC_MQX_BYTE(1) QADC_MQX_BYTE(2) QADC_MQX_BYTE(3)
#undef QADC_MQX_BYTE
#undef QADC_MQX_READ
        }
        return a;
    };
    // one iteration over U tiles: v = the tiles' vectors (zeros where not loaded), tt = first tile, FULL = every lane holds CPL codes
    auto consume = [&](const u32x4_t (&v)[U], uint32_t tt, auto full) {
        Row sums[U * CPL];
        uint32_t all = kTop;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t d[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
            const uint32_t e = (tt + u * G) * kMQWG + tid;
#pragma unroll
            for (int c = 0; c < CPL; ++c) {
                const Row a = code_sums(d + c * DW);
                sums[u * CPL + c] = a;
                const bool live = decltype(full)::value || (tt + u * G < ntiles && e < nvec && e * CPL + c < n);
#pragma unroll
                for (int w = 0; w < ND; ++w) {
                    const uint32_t t = a.d[w] + bias[w];         // field top bit: sum >= bound
                    all &= live ? t : kTop;
                }
            }
        }
        if (__builtin_expect((all & kTop) != kTop, 0)) {         // rare
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int c = 0; c < CPL; ++c) {
                    const uint32_t e = (tt + u * G) * kMQWG + tid;
                    if (!decltype(full)::value && !(tt + u * G < ntiles && e < nvec && e * CPL + c < n)) continue;
#pragma unroll
                    for (int j = 0; j < NQ; ++j) {
                        const uint32_t sj = (sums[u * CPL + c].d[j >> 1] >> (16 * (j & 1))) & 0xffffu;
                        if (sj < bq[j]) {
                            const ScanItem* ij = its + j;
                            emit_candidate(qstates + ij->query, hdr, out + (uint64_t)ij->query * cand_cap, cand_cap,
                                           it.labels, it.key_base, ij->order, it.dup_pos, it.dup_reps, it.pos0 + e * CPL + c, sj);
                        }
                    }
                }
        }
    };
    using full_t = std::integral_constant<bool, true>;
    using part_t = std::integral_constant<bool, false>;
    const uint32_t tiles_full = (n / CPL) / kMQWG;
    uint32_t t0 = bx;
    if (t0 + (U - 1) * G < tiles_full) {                         // software pipeline over the full tiles (see scan_mq_body)
        u32x4_t v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = src[(t0 + u * G) * kMQWG + tid];
        for (;;) {
            const uint32_t tn = t0 + G * U;
            const bool more_full = tn + (U - 1) * G < tiles_full;
            u32x4_t nv[U];
            if (more_full) {
#pragma unroll
                for (int u = 0; u < U; ++u) nv[u] = src[(tn + u * G) * kMQWG + tid];
            }
            consume(v, t0, full_t());
            t0 = tn;
            if (!more_full) break;
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = nv[u];
        }
    }
    for (; t0 < ntiles; t0 += G * U) {
        u32x4_t v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t t = t0 + u * G, e = t * kMQWG + tid;
            v[u] = u32x4_t{0, 0, 0, 0};
            if (t < ntiles && e < nvec) v[u] = src[e];
        }
        consume(v, t0, part_t());
    }
}

// Two builds of the kernel.  NARROW = false: the 8-seat body alone — the flat list's bound levels (every group of a flat
// batch is full but possibly the last).  NARROW = true: both bodies, a group whose seats 4..7 are empty taking the 4-seat
// one — the IVF second phase, whose remainder groups are mostly narrow.  They are separate kernels on purpose: with both
// bodies in it the register allocator lets the pair grow to 104 VGPRs unless 7 waves per SIMD are demanded, and demanded,
// it fits the 8-seat body into 66 with a schedule that costs the FLAT path 5-8 % (1B step 7.77 -> 8.17 ms, 125 M-code
// shard 1.12 -> 1.21 ms: measured against round 2's build on one box) for the 3 % the narrow form gives the IVF path.
template <int M, int U, bool NARROW>
__device__ __forceinline__ void scan_mq_kernel_body(const ScanItem* __restrict__ items, int nitems, const int8_t* __restrict__ qtables,
                                                    QueryState* __restrict__ qstates, CandHeader* __restrict__ hdr, Cand* __restrict__ out,
                                                    uint32_t cand_cap, uint32_t R, uint32_t ngroups) {
    // sibling-major decode over the query GROUPS (see scan_i8_kernel): groups that read the same tiles share an XCD
    const uint32_t G = gridDim.x / ngroups;
    uint32_t bx, grp;
    if ((G & 7u) == 0) {
        const uint32_t r = blockIdx.x >> 3;
        grp = r % ngroups;
        bx = (r / ngroups) * 8u + (blockIdx.x & 7u);
    } else {
        grp = blockIdx.x % ngroups;
        bx = blockIdx.x / ngroups;
    }
    const int first_item = (int)grp * kMQ;
    const int nq = min(kMQ, nitems - first_item);            // queries of this group (>= 1)
    const ScanItem* __restrict__ its = items + first_item;
    const ScanItem it = its[0];                              // codes / n / pos0 / labels / key_base / dup_*: shared
    if (it.n == 0) return;                                   // (device-planned launches are sized for the worst case: no such group)
    lds_base_is_zero();
    if (NARROW) {
        // seats are filled from 0 upward (a remainder group of the IVF second phase is mostly short); nlive = 1 + the highest
        // live seat, so that a form never drops a seat whatever the planner did
        int nlive = 0;
        for (int j = 0; j < nq; ++j) nlive = its[j].n != 0 ? j + 1 : nlive;
        if (nlive <= 2) {
            scan_mq_body_x<M, U, 2>(its, it, min(nq, 2), bx, G, qtables, qstates, hdr, out, cand_cap, R);
            return;
        }
        if (nlive <= 4) {
            scan_mq_body<M, U, 4, true>(its, it, min(nq, 4), bx, G, qtables, qstates, hdr, out, cand_cap, R);
            return;
        }
        if (nlive <= 6) {
            scan_mq_body_x<M, U, 6>(its, it, min(nq, 6), bx, G, qtables, qstates, hdr, out, cand_cap, R);
            return;
        }
    }
    scan_mq_body<M, U, 8, NARROW && true>(its, it, nq, bx, G, qtables, qstates, hdr, out, cand_cap, R);
}

template <int M, int U>
__global__ __launch_bounds__(kMQWG) void scan_i8_mq_kernel(
    const ScanItem* __restrict__ items, int nitems, const int8_t* __restrict__ qtables,
    QueryState* __restrict__ qstates, CandHeader* __restrict__ hdr, Cand* __restrict__ out, uint32_t cand_cap,
    uint32_t R, uint32_t ngroups) {
    scan_mq_kernel_body<M, U, false>(items, nitems, qtables, qstates, hdr, out, cand_cap, R, ngroups);
}

// (7 waves per SIMD asked for: each of the two bodies fits 68 VGPRs by itself; without the demand the occupancy the
// kernel's latency hiding was tuned for — 7 waves per SIMD — drops to 4)
template <int M, int U>
__global__ __launch_bounds__(kMQWG, 7) void scan_i8_mq_narrow_kernel(
    const ScanItem* __restrict__ items, int nitems, const int8_t* __restrict__ qtables,
    QueryState* __restrict__ qstates, CandHeader* __restrict__ hdr, Cand* __restrict__ out, uint32_t cand_cap,
    uint32_t R, uint32_t ngroups) {
    scan_mq_kernel_body<M, U, true>(items, nitems, qtables, qstates, hdr, out, cand_cap, R, ngroups);
}

template <int M>
static void launch_scan_mq_m(const ScanItem* d_items, int nitems, int wgs_per_group, const int8_t* d_qtables,
                             QueryState* d_qs, CandHeader* d_hdr, Cand* d_cands, uint32_t cand_cap, uint32_t R,
                             hipStream_t stream, int narrow) {
    const uint32_t ngroups = (uint32_t)(nitems + kMQ - 1) / kMQ;
    if (narrow)
        hipLaunchKernelGGL((scan_i8_mq_narrow_kernel<M, 2>), dim3(ngroups * (uint32_t)wgs_per_group), dim3(kMQWG), M * 256 + 64,
                           stream, d_items, nitems, d_qtables, d_qs, d_hdr, d_cands, cand_cap, R, ngroups);
    else
        hipLaunchKernelGGL((scan_i8_mq_kernel<M, 2>), dim3(ngroups * (uint32_t)wgs_per_group), dim3(kMQWG), M * 256 + 64,
                           stream, d_items, nitems, d_qtables, d_qs, d_hdr, d_cands, cand_cap, R, ngroups);
}

// Runs of the launch must all cover the same codes (same codes / n / pos0 / labels / key_base / dup_*): the
// planner guarantees it.  Groups of up to 8 consecutive runs share one pass.
void launch_scan_i8_mq(int M, const ScanItem* d_items, int nitems, int wgs_per_group, const int8_t* d_qtables,
                       QueryState* d_qs, CandHeader* d_hdr, Cand* d_cands, uint32_t cand_cap, uint32_t R,
                       hipStream_t stream, int narrow) {
    if (M == 16) launch_scan_mq_m<16>(d_items, nitems, wgs_per_group, d_qtables, d_qs, d_hdr, d_cands, cand_cap, R, stream, narrow);
    else         launch_scan_mq_m<32>(d_items, nitems, wgs_per_group, d_qtables, d_qs, d_hdr, d_cands, cand_cap, R, stream, narrow);
}

// ---------------------------------------------------------------------------------------------
// Small-run variant (IVF partitions, early bound levels): same pair-fused lookup, but the byte tables
// are NOT bank-replicated — 2 KiB (16x4) / 4 KiB (32x4) of LDS and a trivial build, 256-thread
// workgroups, so many workgroups per CU overlap their item/table/histogram fetch latencies.  A table
// spans 64 dwords = 2 per bank, so a lookup is at worst a 2-way bank conflict; that costs LDS cycles
// the streaming kernel cannot afford at 6 TB/s but a run of a few 10^4 codes is latency-bound anyway.
// ---------------------------------------------------------------------------------------------
template <int M, int SU>
__global__ __launch_bounds__(256) void scan_i8_small_kernel(const ScanItem* __restrict__ items,
                                                            const int8_t* __restrict__ qtables,
                                                            QueryState* __restrict__ qstates, CandHeader* __restrict__ hdr,
                                                            Cand* __restrict__ out, uint32_t cand_cap, uint32_t R) {
    constexpr int CS = M / 2, DW = M / 8, CPL = 16 / CS;
    __shared__ __attribute__((aligned(16))) unsigned char ptab[CS * 256];
    __shared__ __attribute__((aligned(16))) unsigned char tq[M * 16];
    __shared__ uint32_t lhist[128];
    __shared__ uint32_t lbound;
    const ScanItem it = items[blockIdx.y];
    QueryState* qs = qstates + it.query;
    out += (uint64_t)it.query * cand_cap;
    const uint32_t tid = threadIdx.x;
    if (tid < M * 4) reinterpret_cast<uint32_t*>(tq)[tid] =
        reinterpret_cast<const uint32_t*>(qtables + (uint64_t)it.table * (M * 16))[tid];
    __syncthreads();
    for (int e = tid; e < CS * 256; e += 256) {
        const int b = e >> 8, x = e & 255;
        ptab[e] = (unsigned char)(tq[(2 * b) * 16 + (x & 15)] + tq[(2 * b + 1) * 16 + (x >> 4)]);
    }
    const uint32_t bound = prefix_bound(qs, it.order >> 16, R, lhist, &lbound);   // syncs inside

    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    typedef const __attribute__((address_space(1))) u32x4* gvec_t;
    const gvec_t src = (gvec_t)(uintptr_t)it.codes;
    const uint32_t n = it.n;
    const uint32_t nvec = (n + CPL - 1) / CPL;
    const uint32_t stride = gridDim.x * 256;
    for (uint32_t e0 = blockIdx.x * 256 + tid; e0 < nvec; e0 += SU * stride) {
        u32x4 v[SU];
        uint32_t e[SU];
#pragma unroll
        for (int u = 0; u < SU; ++u) {
            e[u] = e0 + u * stride;
            v[u] = u32x4{0, 0, 0, 0};
            if (e[u] < nvec) v[u] = __builtin_nontemporal_load(src + e[u]);
            else e[u] = 0xffffffffu;
        }
        uint32_t cand[SU * CPL];
        uint32_t best = 127u;
#pragma unroll
        for (int u = 0; u < SU; ++u) {
            const uint32_t d[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
            for (int c = 0; c < CPL; ++c) {
                uint32_t sum = 0;
#pragma unroll
                for (int b = 0; b < CS; ++b) {
                    const uint32_t w = d[c * DW + (b >> 2)];
                    sum += ptab[b * 256 + ((w >> (8 * (b & 3))) & 0xffu)];
                }
                const bool live = e[u] != 0xffffffffu && e[u] * CPL + c < n;
                cand[u * CPL + c] = live ? min(sum, 127u) : 127u;
                best = min(best, cand[u * CPL + c]);
            }
        }
        if (__builtin_expect(best < bound, 0)) {
#pragma unroll
            for (int u = 0; u < SU; ++u)
#pragma unroll
                for (int c = 0; c < CPL; ++c)
                    if (cand[u * CPL + c] < bound)
                        emit_candidate(qs, hdr, out, cand_cap, it.labels, it.key_base, it.order, it.dup_pos, it.dup_reps,
                                       it.pos0 + e[u] * CPL + c, cand[u * CPL + c]);
        }
    }
}

void launch_scan_i8_small(int M, const ScanItem* d_items, int nitems, int wgs_per_item, const int8_t* d_qtables,
                          QueryState* d_qs, CandHeader* d_hdr, Cand* d_cands, uint32_t cap_per_query, uint32_t R,
                          hipStream_t stream) {
    const dim3 grid(wgs_per_item, nitems), block(256);
    // 4 vectors (64 B) in flight per lane: these runs are latency-bound
    if (M == 16) hipLaunchKernelGGL((scan_i8_small_kernel<16, 4>), grid, block, 0, stream, d_items, d_qtables, d_qs, d_hdr, d_cands, cap_per_query, R);
    else         hipLaunchKernelGGL((scan_i8_small_kernel<32, 4>), grid, block, 0, stream, d_items, d_qtables, d_qs, d_hdr, d_cands, cap_per_query, R);
}

template <int M, bool NT, bool CHUNK, bool PROBE>
static void launch_scan_variant(dim3 grid, hipStream_t stream, const ScanItem* d_items, const int8_t* d_qtables,
                                QueryState* d_qs, CandHeader* d_hdr, Cand* d_cands, uint32_t cand_cap, uint32_t R,
                                uint32_t sib_items) {
    auto k = &scan_i8_kernel<M, NT, CHUNK, PROBE>;
    static std::atomic<uint64_t> done{0};
    ensure_dynamic_lds(reinterpret_cast<const void*>(k), ScanCfg<M>::LDS_BYTES, done);
    hipLaunchKernelGGL(k, grid, dim3(kWG), ScanCfg<M>::LDS_BYTES, stream, d_items, d_qtables, d_qs, d_hdr, d_cands, cand_cap, R, sib_items);
}

template <int PLANES, bool NT, bool CHUNK, bool PROBE>
static void launch_split_variant(dim3 grid, hipStream_t stream, const ScanItem* d_items, const int8_t* d_qtables,
                                 QueryState* d_qs, CandHeader* d_hdr, Cand* d_cands, uint32_t cand_cap, uint32_t R,
                                 const uint8_t* d_plane_sel, unsigned long long* d_surv) {
    auto k = &scan_i8_split_kernel<PLANES, NT, CHUNK, PROBE>;
    static std::atomic<uint64_t> done{0};
    ensure_dynamic_lds(reinterpret_cast<const void*>(k), ScanCfg<16>::LDS_BYTES, done);
    hipLaunchKernelGGL(k, grid, dim3(kWG), ScanCfg<16>::LDS_BYTES, stream, d_items, d_qtables, d_qs, d_hdr, d_cands, cand_cap, R,
                       d_plane_sel, d_surv);
}

template <int NS, bool NT, bool CHUNK, bool PROBE>
static void launch_nib_variant(dim3 grid, hipStream_t stream, const ScanItem* d_items, const int8_t* d_qtables,
                               QueryState* d_qs, CandHeader* d_hdr, Cand* d_cands, uint32_t cand_cap, uint32_t R,
                               const uint8_t* d_nib_sel, unsigned long long* d_surv) {
    auto k = &scan_i8_nib_kernel<NS, NT, CHUNK, PROBE>;
    static std::atomic<uint64_t> done{0};
    ensure_dynamic_lds(reinterpret_cast<const void*>(k), ScanCfg<16>::LDS_BYTES, done);
    hipLaunchKernelGGL(k, grid, dim3(kWG), ScanCfg<16>::LDS_BYTES, stream, d_items, d_qtables, d_qs, d_hdr, d_cands, cand_cap, R,
                       d_nib_sel, d_surv);
}

template <int NSP, bool NT, bool CHUNK, bool PROBE>
static void launch_bkt_variant(dim3 grid, hipStream_t stream, const ScanItem* d_items, const int8_t* d_qtables,
                               QueryState* d_qs, CandHeader* d_hdr, Cand* d_cands, uint32_t cand_cap, uint32_t R,
                               const uint8_t* d_bkt_sel, unsigned long long* d_surv) {
    auto k = &scan_i8_bkt_kernel<NSP, NT, CHUNK, PROBE>;
    static std::atomic<uint64_t> done{0};
    ensure_dynamic_lds(reinterpret_cast<const void*>(k), ScanCfg<16>::LDS_BYTES, done);
    hipLaunchKernelGGL(k, grid, dim3(kWG), ScanCfg<16>::LDS_BYTES, stream, d_items, d_qtables, d_qs, d_hdr, d_cands, cand_cap, R,
                       d_bkt_sel, d_surv);
}

template <int NSP, bool NT, bool CHUNK, bool PROBE>
static void launch_bktw_variant(dim3 grid, hipStream_t stream, const ScanItem* d_items, const int8_t* d_qtables,
                                QueryState* d_qs, CandHeader* d_hdr, Cand* d_cands, uint32_t cand_cap, uint32_t R,
                                const uint8_t* d_bktw_sel, unsigned long long* d_surv) {
    auto k = &scan_i8_bktw_kernel<NSP, NT, CHUNK, PROBE>;
    static std::atomic<uint64_t> done{0};
    ensure_dynamic_lds(reinterpret_cast<const void*>(k), ScanCfg<16>::LDS_BYTES, done);
    hipLaunchKernelGGL(k, grid, dim3(kWG), ScanCfg<16>::LDS_BYTES, stream, d_items, d_qtables, d_qs, d_hdr, d_cands, cand_cap, R,
                       d_bktw_sel, d_surv);
}

template <int NSP, bool NT, bool CHUNK, bool PROBE, bool QUARTER>
static void launch_bktw_prune_variant(dim3 grid, hipStream_t stream, const ScanItem* d_items, const int8_t* d_qtables,
                                      QueryState* d_qs, CandHeader* d_hdr, Cand* d_cands, uint32_t cand_cap, uint32_t R,
                                      const uint8_t* d_bktw_sel, unsigned long long* d_surv, unsigned long long* d_prune_cnt) {
    auto k = &scan_i8_bktw_prune_kernel<NSP, NT, CHUNK, PROBE, QUARTER>;
    static std::atomic<uint64_t> done{0};
    ensure_dynamic_lds(reinterpret_cast<const void*>(k), ScanCfg<16>::LDS_BYTES, done);
    hipLaunchKernelGGL(k, grid, dim3(kWG), ScanCfg<16>::LDS_BYTES, stream, d_items, d_qtables, d_qs, d_hdr, d_cands, cand_cap, R,
                       d_bktw_sel, d_surv, d_prune_cnt);
}

// variant bits: [2] NT (non-temporal loads)  [3] CHUNK  [4] PROBE (ceiling diagnostic)
// [5] split form (16x4, every run of the launch has ScanItem::split; not with [6]): 5 planes when d_plane_sel5 (the two
//     deferred bytes and the slack of every table) is given, else 6 planes when d_plane_sel (the deferred byte of every
//     table) is, else 7 (launch_plane_choice / launch_select_kth write both); d_surv: survivor counter or nullptr
//     nib_ns = 8, 9 or 10 with d_nib_sel (ScanItem::split of every run points into the nibble-plane copy): the nibble form, before all of these
//     bkt_nsp = 4..7 with d_bkt_sel (every run of the launch is a bucket-form run, LevelLaunch::bkt): the bucket form, before the nibble form
//     bkt_free = 5, bkt_nsp = 3..6, d_bkt_sel = the wide form's choice bytes (LevelLaunch::bktw): the wide form, before all of these
//     ... bkt_prune != 0: its build with the group test (scan_i8_bktw_prune_kernel; d_prune_cnt: its four counters or nullptr;
//     bkt_prune_lanes = 16: kept wave iterations load by 16-lane quarters, any other value: by whole waves)
// [6] sibling-major 1-D launch (every run of the launch covers the same codes; see the kernel's decode).  Other bits: ignored.
void launch_scan_i8(int M, int variant, const ScanItem* d_items, int nitems, int wgs_per_item,
                    const int8_t* d_qtables, QueryState* d_qs, CandHeader* d_hdr, Cand* d_cands, uint32_t cand_cap,
                    uint32_t R, hipStream_t stream, const uint8_t* d_plane_sel, unsigned long long* d_surv,
                    const uint8_t* d_plane_sel5, const uint8_t* d_nib_sel, int nib_ns, const uint8_t* d_bkt_sel, int bkt_nsp, int bkt_free,
                    int bkt_prune, unsigned long long* d_prune_cnt, int bkt_prune_lanes) {
    if (bkt_free == 5) {
        // a wide launch is never anything else: launch_level (qadc_capi.cpp) refuses one whose preconditions do not hold with an error
        // status before it gets here, so a violation is a programming error and must not pass as a level that was silently not scanned
        if (!(M == 16 && (variant & 32) && !(variant & 64) && d_bkt_sel && bkt_nsp >= 3 && bkt_nsp <= 6)) {
            std::fprintf(stderr, "qadc: launch_scan_i8: a wide bucket launch without its preconditions (M %d, variant 0x%x, nsp %d)\n", M, variant, bkt_nsp);
            std::abort();
        }
        const dim3 grid(wgs_per_item, nitems);
#define QADC_BKTW_ARGS grid, stream, d_items, d_qtables, d_qs, d_hdr, d_cands, cand_cap, R, d_bkt_sel, d_surv
#define QADC_BKTW(NSP, PR)                                                        \
    switch ((variant >> 2) & 3) {                                                 \
        case 0: launch_bktw_variant<NSP, false, false, PR>(QADC_BKTW_ARGS); break; \
        case 1: launch_bktw_variant<NSP, true, false, PR>(QADC_BKTW_ARGS); break;  \
        case 2: launch_bktw_variant<NSP, false, true, PR>(QADC_BKTW_ARGS); break;  \
        default: launch_bktw_variant<NSP, true, true, PR>(QADC_BKTW_ARGS); break;  \
    }
#define QADC_BKTWPQ(NSP, PR, QU)                                                                           \
    switch ((variant >> 2) & 3) {                                                                         \
        case 0: launch_bktw_prune_variant<NSP, false, false, PR, QU>(QADC_BKTW_ARGS, d_prune_cnt); break; \
        case 1: launch_bktw_prune_variant<NSP, true, false, PR, QU>(QADC_BKTW_ARGS, d_prune_cnt); break;  \
        case 2: launch_bktw_prune_variant<NSP, false, true, PR, QU>(QADC_BKTW_ARGS, d_prune_cnt); break;  \
        default: launch_bktw_prune_variant<NSP, true, true, PR, QU>(QADC_BKTW_ARGS, d_prune_cnt); break;  \
    }
#define QADC_BKTWP(NSP, PR) \
    if (bkt_prune_lanes == 16) { QADC_BKTWPQ(NSP, PR, true) } else { QADC_BKTWPQ(NSP, PR, false) }
        if (bkt_prune) {
            if (bkt_nsp == 3) {
                if (variant & 16) { QADC_BKTWP(3, true) } else { QADC_BKTWP(3, false) }
            } else if (bkt_nsp == 4) {
                if (variant & 16) { QADC_BKTWP(4, true) } else { QADC_BKTWP(4, false) }
            } else if (bkt_nsp == 5) {
                if (variant & 16) { QADC_BKTWP(5, true) } else { QADC_BKTWP(5, false) }
            } else {
                if (variant & 16) { QADC_BKTWP(6, true) } else { QADC_BKTWP(6, false) }
            }
        } else if (bkt_nsp == 3) {
            if (variant & 16) { QADC_BKTW(3, true) } else { QADC_BKTW(3, false) }
        } else if (bkt_nsp == 4) {
            if (variant & 16) { QADC_BKTW(4, true) } else { QADC_BKTW(4, false) }
        } else if (bkt_nsp == 5) {
            if (variant & 16) { QADC_BKTW(5, true) } else { QADC_BKTW(5, false) }
        } else {
            if (variant & 16) { QADC_BKTW(6, true) } else { QADC_BKTW(6, false) }
        }
#undef QADC_BKTW_ARGS
#undef QADC_BKTW
#undef QADC_BKTWP
#undef QADC_BKTWPQ
        return;
    }
    if (M == 16 && (variant & 32) && !(variant & 64) && d_bkt_sel && bkt_nsp >= 4 && bkt_nsp <= 7) {
        const dim3 grid(wgs_per_item, nitems);
#define QADC_BKT_ARGS grid, stream, d_items, d_qtables, d_qs, d_hdr, d_cands, cand_cap, R, d_bkt_sel, d_surv
#define QADC_BKT(NSP, PR)                                                       \
    switch ((variant >> 2) & 3) {                                               \
        case 0: launch_bkt_variant<NSP, false, false, PR>(QADC_BKT_ARGS); break; \
        case 1: launch_bkt_variant<NSP, true, false, PR>(QADC_BKT_ARGS); break;  \
        case 2: launch_bkt_variant<NSP, false, true, PR>(QADC_BKT_ARGS); break;  \
        default: launch_bkt_variant<NSP, true, true, PR>(QADC_BKT_ARGS); break;  \
    }
        if (bkt_nsp == 4) {
            if (variant & 16) { QADC_BKT(4, true) } else { QADC_BKT(4, false) }
        } else if (bkt_nsp == 5) {
            if (variant & 16) { QADC_BKT(5, true) } else { QADC_BKT(5, false) }
        } else if (bkt_nsp == 6) {
            if (variant & 16) { QADC_BKT(6, true) } else { QADC_BKT(6, false) }
        } else {
            if (variant & 16) { QADC_BKT(7, true) } else { QADC_BKT(7, false) }
        }
#undef QADC_BKT_ARGS
#undef QADC_BKT
        return;
    }
    if (M == 16 && (variant & 32) && !(variant & 64) && d_nib_sel && nib_ns >= 8 && nib_ns <= 10) {
        const dim3 grid(wgs_per_item, nitems);
#define QADC_NIB_ARGS grid, stream, d_items, d_qtables, d_qs, d_hdr, d_cands, cand_cap, R, d_nib_sel, d_surv
#define QADC_NIB(NS, PR)                                                       \
    switch ((variant >> 2) & 3) {                                              \
        case 0: launch_nib_variant<NS, false, false, PR>(QADC_NIB_ARGS); break; \
        case 1: launch_nib_variant<NS, true, false, PR>(QADC_NIB_ARGS); break;  \
        case 2: launch_nib_variant<NS, false, true, PR>(QADC_NIB_ARGS); break;  \
        default: launch_nib_variant<NS, true, true, PR>(QADC_NIB_ARGS); break;  \
    }
        if (nib_ns == 8) {
            if (variant & 16) { QADC_NIB(8, true) } else { QADC_NIB(8, false) }
        } else if (nib_ns == 9) {
            if (variant & 16) { QADC_NIB(9, true) } else { QADC_NIB(9, false) }
        } else {
            if (variant & 16) { QADC_NIB(10, true) } else { QADC_NIB(10, false) }
        }
#undef QADC_NIB_ARGS
#undef QADC_NIB
        return;
    }
    if (M == 16 && (variant & 32) && !(variant & 64)) {
        const dim3 grid(wgs_per_item, nitems);
#define QADC_SPLIT_ARGS grid, stream, d_items, d_qtables, d_qs, d_hdr, d_cands, cand_cap, R, d_plane_sel, d_surv
#define QADC_SPLIT(PL, PR)                                                       \
    switch ((variant >> 2) & 3) {                                                \
        case 0: launch_split_variant<PL, false, false, PR>(QADC_SPLIT_ARGS); break; \
        case 1: launch_split_variant<PL, true, false, PR>(QADC_SPLIT_ARGS); break;  \
        case 2: launch_split_variant<PL, false, true, PR>(QADC_SPLIT_ARGS); break;  \
        default: launch_split_variant<PL, true, true, PR>(QADC_SPLIT_ARGS); break;  \
    }
        if (d_plane_sel5) {
            d_plane_sel = d_plane_sel5;                          // (the kernel's one selection argument)
            if (variant & 16) { QADC_SPLIT(5, true) } else { QADC_SPLIT(5, false) }
        } else if (d_plane_sel) {
            if (variant & 16) { QADC_SPLIT(6, true) } else { QADC_SPLIT(6, false) }
        } else {
            if (variant & 16) { QADC_SPLIT(7, true) } else { QADC_SPLIT(7, false) }
        }
#undef QADC_SPLIT_ARGS
#undef QADC_SPLIT
        return;
    }
    const bool sib = (variant & 64) != 0;
    const dim3 grid = sib ? dim3((unsigned)wgs_per_item * (unsigned)nitems) : dim3(wgs_per_item, nitems);
    const uint32_t sib_items = sib ? (uint32_t)nitems : 0u;
#define QADC_ARGS grid, stream, d_items, d_qtables, d_qs, d_hdr, d_cands, cand_cap, R, sib_items
#define QADC_DISPATCH_P(MM, PR)                                             \
    switch ((variant >> 2) & 3) {                                           \
        case 0: launch_scan_variant<MM, false, false, PR>(QADC_ARGS); break; \
        case 1: launch_scan_variant<MM, true, false, PR>(QADC_ARGS); break;  \
        case 2: launch_scan_variant<MM, false, true, PR>(QADC_ARGS); break;  \
        default: launch_scan_variant<MM, true, true, PR>(QADC_ARGS); break;  \
    }
#define QADC_DISPATCH(MM)                                                   \
    if (variant & 16) { QADC_DISPATCH_P(MM, true) } else { QADC_DISPATCH_P(MM, false) }
    if (M == 16) { QADC_DISPATCH(16) } else { QADC_DISPATCH(32) }
#undef QADC_DISPATCH
#undef QADC_DISPATCH_P
#undef QADC_ARGS
}

// ---------------------------------------------------------------------------------------------
// Device-side ordering of the candidates: the host replay needs them in scan order
// (level, assign slot, position).  A query's region is already grouped by level — slots are handed
// out by an atomic counter and the levels are separate, stream-ordered launches — so each level's
// segment (<= R * growth entries, typically a few hundred) is sorted by ONE WAVE with a barrier-free
// bitonic network in its own LDS slice, all levels concurrently.  Segments above 512 entries fall
// back to a workgroup-wide bitonic sort of the whole region.
// ---------------------------------------------------------------------------------------------
constexpr uint32_t kSegCap = 512;                        // entries one wave sorts: 4 KiB keys + 4 KiB payload per wave

__device__ __forceinline__ uint64_t cand_sort_key(const Cand& c, uint32_t idx) {
    const uint64_t ord = ((uint64_t)((c.order >> 16) & 15u) << 14) | (c.order & 0x3fffu);
    return (ord << 46) | ((uint64_t)c.pos << 14) | idx;
}

__device__ __forceinline__ void wave_lds_sync() {
    // LDS operations of one wave execute in order; this only stops the compiler from moving them
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// Bitonic sort of 512 u64 keys held by one wave, 8 per lane, element e = r*64 + lane.  Exchanges at distance
// >= 64 are register swaps inside a lane, shorter ones are wave shuffles: no LDS round trips, no barriers.
__device__ __forceinline__ void wave_sort512(uint64_t (&v)[8], uint32_t lane) {
#pragma unroll
    for (uint32_t k = 2; k <= 512; k <<= 1) {
#pragma unroll
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            if (j >= 64) {
                const uint32_t jr = j >> 6;
#pragma unroll
                for (uint32_t r = 0; r < 8; ++r) {
                    if ((r & jr) == 0) {
                        const bool asc = (((r << 6) | lane) & k) == 0;
                        const uint64_t a = v[r], b = v[r | jr];
                        const bool sw = (a > b) == asc;
                        v[r] = sw ? b : a;
                        v[r | jr] = sw ? a : b;
                    }
                }
            } else {
                const bool lower = (lane & j) == 0;
#pragma unroll
                for (uint32_t r = 0; r < 8; ++r) {
                    const bool asc = (((r << 6) | lane) & k) == 0;
                    const uint64_t a = v[r];
                    const uint64_t b = ((uint64_t)__shfl_xor((uint32_t)(a >> 32), j, 64) << 32) | __shfl_xor((uint32_t)a, j, 64);
                    const bool keep_min = lower == asc;
                    v[r] = keep_min ? (a < b ? a : b) : (a > b ? a : b);
                }
            }
        }
    }
}

__device__ __forceinline__ void write_query_out(QueryOut* __restrict__ o, const QueryState* qs, uint32_t off, uint32_t flags) {
    o->count = qs->count;
    o->reps = qs->reps;
    o->flags = flags;
    o->out_off = off;
    o->qmin = qs->qmin;
    o->qmax = qs->qmax;
}

__global__ __launch_bounds__(1024) void sort_cands_kernel(QueryState* __restrict__ qstates, const Cand* __restrict__ cands,
                                                          uint32_t cap, int nq, QueryOut* __restrict__ qout,
                                                          uint64_t* __restrict__ out_entries, uint32_t out_cap,
                                                          CandHeader* __restrict__ hdr,
                                                          uint64_t* __restrict__ dev_entries) {
    // all LDS in the dynamic region (keeps the 8-byte key array naturally aligned)
    uint64_t* lkey = reinterpret_cast<uint64_t*>(smem);
    uint32_t* scan = reinterpret_cast<uint32_t*>(smem + kSortCap * 8);   // [1024] + misc
    uint32_t& s_off = scan[1024];
    uint32_t* seg_cnt = scan + 1025;                         // [16]
    uint32_t* seg_off = scan + 1041;                         // [17]
    uint32_t* seg_reps = scan + 1058;                        // [16] then exclusive prefix
    uint32_t& s_fast = scan[1074];
    const int q = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    QueryState* qs = qstates + q;
    const uint32_t n = qs->count;
    const uint32_t limit = min(cap, kSortCap);
    if (n > limit) {                                             // host sorts this query's region
        if (tid == 0) write_query_out(qout + q, qs, 0, qs->flags);
        return;
    }
    // offset of this query in the compact output = candidates (+ replays) of the device-sorted queries before it
    uint32_t part = 0;
    for (int p = tid; p < q; p += 1024) {
        const uint32_t c = qstates[p].count;
        if (c <= limit) part += c + qstates[p].reps;
    }
    scan[tid] = part;
    // entries per level = sum of the level's value histogram (wave w <-> level w)
    {
        uint32_t c = qs->hist[wave * 128 + lane] + qs->hist[wave * 128 + 64 + lane];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d, 64);
        if (lane == 0) seg_cnt[wave] = c;
    }
    __syncthreads();
    for (int d = 512; d >= 1; d >>= 1) {
        if (tid < d) scan[tid] += scan[tid + d];
        __syncthreads();
    }
    if (tid == 0) {
        s_off = scan[0];
        uint32_t run = 0, fast = 1;
        for (int l = 0; l < kMaxLevels; ++l) {
            seg_off[l] = run;
            run += seg_cnt[l];
            if (seg_cnt[l] > kSegCap) fast = 0;
        }
        seg_off[kMaxLevels] = run;
        s_fast = (fast && run == n) ? 1u : 0u;
    }
    __syncthreads();
    const uint32_t off = s_off;
    const Cand* __restrict__ region = cands + (uint64_t)q * cap;

    if (s_fast) {
        // ---- one wave per level segment, no workgroup barriers in the sort ----
        uint64_t* wkey = lkey + (size_t)wave * (2 * kSegCap);   // [kSegCap] sort keys
        uint64_t* wpay = wkey + kSegCap;                          // [kSegCap] payload: key | (val | replays << 8) << 32
        const uint32_t s0 = seg_off[wave], ns = seg_cnt[wave];
        // keys in registers (element e = r*64 + lane), payload in LDS indexed by the entry's position in the segment
        uint64_t v[8];
#pragma unroll
        for (uint32_t r = 0; r < 8; ++r) {
            const uint32_t i = r * 64 + lane;
            uint64_t k = ~0ull;
            if (i < ns) {
                const Cand c = region[s0 + i];
                k = cand_sort_key(c, i);
                wpay[i] = (uint64_t)c.key | ((uint64_t)(c.val | (((c.order >> 20) & 15u) << 8)) << 32) |
                          ((uint64_t)(c.order & 0x3fffu) << 48);   // key | value | replays << 40 | assign slot << 48
            }
            v[r] = k;
        }
        if (ns > 1) wave_sort512(v, lane);
#pragma unroll
        for (uint32_t r = 0; r < 8; ++r) wkey[r * 64 + lane] = v[r];
        wave_lds_sync();
        const uint32_t n2 = 512;
        // padding-lane replays: lane owns sorted entries [lane*chunk, (lane+1)*chunk) of the segment
        const uint32_t chunk = n2 / 64;
        const uint32_t b0 = min(ns, lane * chunk), b1 = min(ns, (lane + 1) * chunk);
        uint32_t myreps = 0;
        for (uint32_t i = b0; i < b1; ++i) myreps += (uint32_t)(wpay[wkey[i] & 0x3fffu] >> 40) & 15u;
        uint32_t incl = myreps;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t o = __shfl_up(incl, d, 64);
            if (lane >= d) incl += o;
        }
        if (lane == 63) seg_reps[wave] = incl;
        __syncthreads();
        if (tid == 0) {
            uint32_t run = 0;
            for (int l = 0; l < kMaxLevels; ++l) {
                const uint32_t r = seg_reps[l];
                seg_reps[l] = run;
                run += r;
            }
        }
        __syncthreads();
        uint32_t w = off + s0 + seg_reps[wave] + b0 + (incl - myreps);
        for (uint32_t i = b0; i < b1; ++i) {
            const uint64_t pay = wpay[wkey[i] & 0x3fffu];
            const uint32_t reps = 1u + ((uint32_t)(pay >> 40) & 15u);
            for (uint32_t r = 0; r < reps; ++r, ++w) {
                // entry = key | value << 32 | assign slot << 40
                if (w < out_cap) {
                    const uint64_t en = (pay & 0xffffffffffull) | ((pay >> 48) << 40);
                    out_entries[w] = en;
                    if (dev_entries) dev_entries[w] = en;        // copy in device memory for replay_heap_kernel
                } else {
                    atomicAdd(&hdr->out_overflow, 1u);
                }
            }
        }
        if (tid == 0) {
            write_query_out(qout + q, qs, off, qs->flags | 4u);
            qs->out_off = off;
            qs->flags |= 4u;
        }
        return;
    }

    // ---- fallback: workgroup-wide bitonic sort of the whole region ----
    uint32_t n2 = 1;
    while (n2 < n) n2 <<= 1;
    for (uint32_t i = tid; i < n2; i += 1024) lkey[i] = i < n ? cand_sort_key(region[i], i) : ~0ull;
    __syncthreads();
    for (uint32_t k = 2; k <= n2; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t i = tid; i < n2; i += 1024) {
                const uint32_t p = i ^ j;
                if (p > i) {
                    const uint64_t a = lkey[i], b = lkey[p];
                    if ((a > b) == ((i & k) == 0)) { lkey[i] = b; lkey[p] = a; }
                }
            }
            __syncthreads();
        }
    // expand padding-lane replays while writing: thread t owns sorted entries [t*chunk, (t+1)*chunk)
    const uint32_t chunk = (n2 + 1023) / 1024;
    const uint32_t b0 = min(n, tid * chunk), b1 = min(n, (tid + 1) * chunk);
    uint32_t myreps = 0;
    for (uint32_t i = b0; i < b1; ++i) myreps += (region[lkey[i] & 0x3fffu].order >> 20) & 15u;
    scan[tid] = myreps;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const uint32_t o = tid >= d ? scan[tid - d] : 0;
        __syncthreads();
        scan[tid] += o;
        __syncthreads();
    }
    uint32_t w = off + b0 + (scan[tid] - myreps);
    for (uint32_t i = b0; i < b1; ++i) {
        const Cand c = region[lkey[i] & 0x3fffu];
        const uint32_t reps = 1u + ((c.order >> 20) & 15u);
        for (uint32_t r = 0; r < reps; ++r, ++w) {
            if (w < out_cap) {
                const uint64_t en = (uint64_t)c.key | ((uint64_t)(c.val & 0xffu) << 32) | ((uint64_t)(c.order & 0x3fffu) << 40);
                out_entries[w] = en;
                if (dev_entries) dev_entries[w] = en;
            } else {
                atomicAdd(&hdr->out_overflow, 1u);
            }
        }
    }
    if (tid == 0) {
        write_query_out(qout + q, qs, off, qs->flags | 4u);
        qs->out_off = off;
        qs->flags |= 4u;
    }
}

// ---------------------------------------------------------------------------------------------
// The reference's heap on the device (kv_binheap<unsigned,int8_t>::push, binheap.hpp:75-116): one wave per
// query replays the query's ordered candidate stream through a binary max-heap of capacity R kept in LDS —
// sentinel (0,127) first (db_query_4.cpp:276), then every entry in scan order.  The pushes of one query are
// inherently sequential (lane 0 executes them; the other lanes stage the stream through LDS 64 entries at a
// time and write the result out), but thousands of queries replay side by side, which is what an IVF batch
// needs: the host then only copies R entries per query instead of assembling and replaying the streams.
// Same arrays as the host replay (qadc_heap.hpp): appended and bubbled up past strictly smaller parents while
// there is room; afterwards accepted only if strictly below the root, sinking with the left child preferred on
// ties and stopping at a child <= the value.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void replay_heap_kernel(const QueryState* __restrict__ qstates,
                                                         const uint64_t* __restrict__ dev_entries, uint32_t out_cap,
                                                         uint32_t R, uint64_t* __restrict__ heaps,
                                                         uint32_t* __restrict__ heap_sizes) {
    uint64_t* hv = reinterpret_cast<uint64_t*>(smem);            // [R]  key | value << 32
    uint64_t* buf = hv + R;                                      // [64] staged stream entries
    const int q = blockIdx.x;
    const uint32_t lane = threadIdx.x;
    const QueryState* qs = qstates + q;
    const uint32_t flags = qs->flags;
    if (!(flags & 4u) || (uint64_t)qs->out_off + qs->count + qs->reps > out_cap) {   // not ordered on the device: host replays
        if (lane == 0) heap_sizes[q] = 0xffffffffu;
        return;
    }
    if (flags & 1u) {                                            // qmax too high: the reference exits, no result
        if (lane == 0) heap_sizes[q] = 0;
        return;
    }
    const uint32_t n = qs->count + qs->reps;
    const uint64_t* __restrict__ src = dev_entries + qs->out_off;
    uint32_t size = 0;                                           // meaningful on lane 0
    auto val_of = [](uint64_t e) { return (int32_t)((e >> 32) & 0xffu); };
    auto push = [&](uint64_t e) {
        const int32_t value = val_of(e);
        if (size != R) {
            uint32_t i = size++;
            while (i != 0) {
                const uint32_t parent = (i - 1) / 2;
                const uint64_t pe = hv[parent];
                if (!(value > val_of(pe))) break;
                hv[i] = pe;
                i = parent;
            }
            hv[i] = e;
            return;
        }
        if (!(value < val_of(hv[0]))) return;
        uint32_t i = 0;
        for (;;) {
            const uint32_t l = 2 * i + 1;
            if (l >= size) break;
            uint64_t ce = hv[l];
            uint32_t c = l;
            if (l + 1 < size) {
                const uint64_t re = hv[l + 1];
                if (val_of(re) > val_of(ce)) { ce = re; c = l + 1; }
            }
            if (val_of(ce) <= value) break;
            hv[i] = ce;
            i = c;
        }
        hv[i] = e;
    };
    if (lane == 0) push((uint64_t)127 << 32);                    // the sentinel: key 0, value 127
    for (uint32_t base = 0; base < n; base += 64) {
        const uint32_t m = min(64u, n - base);
        if (lane < m) buf[lane] = src[base + lane] & 0xffffffffffull;   // key | value (assign slot dropped)
        wave_lds_sync();
        if (lane == 0)
            for (uint32_t j = 0; j < m; ++j) push(buf[j]);
        wave_lds_sync();
    }
    size = __shfl(size, 0, 64);
    for (uint32_t i = lane; i < size; i += 64) heaps[(uint64_t)q * R + i] = hv[i];
    if (lane == 0) heap_sizes[q] = size;
}

void launch_replay_heap(const QueryState* d_qs, const uint64_t* d_entries, uint32_t out_cap, int nq, uint32_t R,
                        uint64_t* d_heaps, uint32_t* d_heap_sizes, hipStream_t stream) {
    hipLaunchKernelGGL(replay_heap_kernel, dim3(nq), dim3(64), (size_t)(R + 64) * 8, stream, d_qs, d_entries, out_cap, R, d_heaps,
                       d_heap_sizes);
}

void launch_sort_cands(QueryState* d_qs, const Cand* d_cands, uint32_t cap_per_query, int nq, QueryOut* d_qout,
                       uint64_t* d_entries, uint32_t out_cap, CandHeader* d_hdr, hipStream_t stream,
                       uint64_t* d_dev_entries) {
    static std::atomic<uint64_t> done{0};
    ensure_dynamic_lds(reinterpret_cast<const void*>(&sort_cands_kernel), kSortCap * 8 + 4352, done);
    hipLaunchKernelGGL(sort_cands_kernel, dim3(nq), dim3(1024), kSortCap * 8 + 4352, stream, d_qs, d_cands, cap_per_query, nq,
                       d_qout, d_entries, out_cap, d_hdr, d_dev_entries);
}

// All candidate values (diagnostic; used by parity tests and checksums at full size).
template <int M>
__global__ __launch_bounds__(kWG) void candidates_i8_kernel(const uint8_t* __restrict__ codes, uint64_t n,
                                                            const int8_t* __restrict__ qtable, int8_t* __restrict__ out) {
    using C = ScanCfg<M>;
    lds_base_is_zero();
    build_pair_tables<M>(qtable);
    __syncthreads();
    const uint32_t tid = threadIdx.x;
    const uint32_t lane_lo = (tid & 31u) * 4u, lane_hi = lane_lo | 0x10000u;
    const uint4* __restrict__ src = reinterpret_cast<const uint4*>(codes);
    const uint64_t nvec = (n + C::CPL - 1) / C::CPL;
    for (uint64_t e = (uint64_t)blockIdx.x * kWG + tid; e < nvec; e += (uint64_t)gridDim.x * kWG) {
        const uint4 v = src[e];
        const uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int c = 0; c < C::CPL; ++c) {
            const uint64_t idx = e * C::CPL + c;
            if (idx < n) out[idx] = (int8_t)min(pair_sum<M>(d + c * C::DW, lane_lo, lane_hi), 127u);
        }
    }
}

void launch_candidates_i8(int M, const uint8_t* d_codes, uint64_t n, const int8_t* d_qtable, int8_t* d_out,
                          hipStream_t stream) {
    const uint64_t nvec = (n + (M == 16 ? 2 : 1) - 1) / (M == 16 ? 2 : 1);
    const int grid = (int)std::min<uint64_t>((nvec + kWG - 1) / kWG, 512);
    if (M == 16) {
        static std::atomic<uint64_t> done{0};
        ensure_dynamic_lds(reinterpret_cast<const void*>(&candidates_i8_kernel<16>), ScanCfg<16>::LDS_BYTES, done);
        hipLaunchKernelGGL(candidates_i8_kernel<16>, dim3(grid), dim3(kWG), ScanCfg<16>::LDS_BYTES, stream, d_codes, n,
                           d_qtable, d_out);
    } else {
        static std::atomic<uint64_t> done{0};
        ensure_dynamic_lds(reinterpret_cast<const void*>(&candidates_i8_kernel<32>), ScanCfg<32>::LDS_BYTES, done);
        hipLaunchKernelGGL(candidates_i8_kernel<32>, dim3(grid), dim3(kWG), ScanCfg<32>::LDS_BYTES, stream, d_codes, n,
                           d_qtable, d_out);
    }
}

// All candidate values of a partition under a SIGNED int8 table, exactly as scan_avx_4<M> adds them (simd_scan.hpp:138-179):
//   lo chain  T[0][p0.lo] (+) T[1][p0.hi] (+) T[4][p2.lo] (+) T[5][p2.hi] ...    hi chain  T[2][p1.lo] (+) T[3][p1.hi] (+) ...
//   cand = hi (+) lo,   (+) = _mm256_adds_epi8: every partial sum saturates to [-128, 127]
// Negative entries exist only when a NaN made the reference build's qmin overshoot finite table entries (qadc_front_nonfinite.h);
// the streaming scan kernels, written for entries in [0, 127] where this equals min(127, sum), are not used for such a query:
// the host replays these values through the reference's block-wise push rule (qadc_capi.cpp: replay_signed_query).
__device__ __forceinline__ int sat_add8(int a, int b) { return max(-128, min(127, a + b)); }

template <int M>
__global__ __launch_bounds__(256) void candidates_i8_signed_kernel(const uint8_t* __restrict__ codes, uint64_t n,
                                                                   const int8_t* __restrict__ qtable, int8_t* __restrict__ out) {
    constexpr int CS = M / 2;
    __shared__ int8_t qt[M * 16];
    for (int i = threadIdx.x; i < M * 16; i += 256) qt[i] = qtable[i];
    __syncthreads();
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        const uint8_t* __restrict__ c = codes + i * CS;
        int lo = 0, hi = 0;
#pragma unroll
        for (int r = 0; r < M / 4; ++r) {
            const uint32_t p0 = c[2 * r], p1 = c[2 * r + 1];
            const int a = qt[(4 * r) * 16 + (p0 & 15u)], b = qt[(4 * r + 1) * 16 + (p0 >> 4)];
            const int cc = qt[(4 * r + 2) * 16 + (p1 & 15u)], d = qt[(4 * r + 3) * 16 + (p1 >> 4)];
            if (r == 0) {
                lo = sat_add8(b, a);
                hi = sat_add8(d, cc);
            } else {
                lo = sat_add8(b, sat_add8(a, lo));
                hi = sat_add8(d, sat_add8(cc, hi));
            }
        }
        out[i] = (int8_t)sat_add8(hi, lo);
    }
}

void launch_candidates_i8_signed(int M, const uint8_t* d_codes, uint64_t n, const int8_t* d_qtable, int8_t* d_out,
                                 hipStream_t stream) {
    const int grid = (int)std::max<uint64_t>(1, std::min<uint64_t>((n + 255) / 256, 2048));
    if (M == 16) hipLaunchKernelGGL(candidates_i8_signed_kernel<16>, dim3(grid), dim3(256), 0, stream, d_codes, n, d_qtable, d_out);
    else         hipLaunchKernelGGL(candidates_i8_signed_kernel<32>, dim3(grid), dim3(256), 0, stream, d_codes, n, d_qtable, d_out);
}

// ---------------------------------------------------------------------------------------------
// float pre-scan of the "starts" (scan_4<M>, query_common.hpp:59-90): the same IEEE adds in the grouping
// sum_mode names (qadc_float_sum.h): 1 = the reference as compiled with its -ffast-math, 0 = source order.
// The 16 lanes-distinct entries of one table sit in 16 consecutive LDS dwords, so every lookup
// instruction (all lanes in the same table) is bank-conflict-free without replication.
// ---------------------------------------------------------------------------------------------
// (of the value's RANK image: everything that is not below FLT_MAX — NaN sums of either sign, +inf — ranks as FLT_MAX, the
// sentinel the reference's heap never lets them replace; qadc_front_nonfinite.h)
__device__ __forceinline__ uint32_t fkey(float f) {
    const uint32_t b = __float_as_uint(qadc_prescan_rank_value(f));
    return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float funkey(uint32_t k) {
    return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu));
}

template <int M, int SM>
__global__ __launch_bounds__(256) void start_scan_f32_kernel(const StartItem* __restrict__ items,
                                                             const float* __restrict__ ftables, float* __restrict__ fc,
                                                             uint64_t fc_stride, const uint32_t* __restrict__ fc_init,
                                                             QueryState* __restrict__ qstates) {
    constexpr int kStage = 1024;                             // survivors staged in LDS per workgroup
    __shared__ float tab[M * 16];
    __shared__ float stage[kStage];
    __shared__ uint32_t stage_n, stage_base;
    __shared__ uint32_t red[8];
    const StartItem it = items[blockIdx.y];
    const float* __restrict__ ft = ftables + (uint64_t)it.table * (M * 16);
    if (threadIdx.x == 0) stage_n = 0;
    for (int i = threadIdx.x; i < M * 16; i += 256) tab[i] = ft[i];
    __syncthreads();
    float* __restrict__ dst = fc + (uint64_t)it.query * fc_stride;
    QueryState* qs = qstates + it.query;
    const float thr = it.filter ? qs->qmax : 0.0f;           // R-th smallest of the sample (phase A)
    const uint32_t base_n = fc_init[2 * it.query], cap = fc_init[2 * it.query + 1];   // survivors go behind the sample
    constexpr int DW = M / 8;
    uint32_t kmin = 0xffffffffu, kmax = 0u;
    const uint32_t stride = gridDim.x * 256;
    // two codes per lane and iteration: two independent float sums in flight
    for (uint32_t i0 = blockIdx.x * 256 + threadIdx.x; i0 < it.n; i0 += 2 * stride) {
        uint32_t d[2][DW];
        bool live[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const uint32_t i = i0 + u * stride;
            live[u] = i < it.n;
#pragma unroll
            for (int w = 0; w < DW; ++w) d[u][w] = 0;
            if (live[u]) {
                // explicit global address space: a pointer read from the item struct is generic otherwise
                if constexpr (M == 16) {
                    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
                    const u32x2 v = ((const __attribute__((address_space(1))) u32x2*)(uintptr_t)it.codes)[i];
                    d[u][0] = v.x; d[u][1] = v.y;
                } else {
                    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
                    const u32x4 v = ((const __attribute__((address_space(1))) u32x4*)(uintptr_t)it.codes)[i];
                    d[u][0] = v.x; d[u][1] = v.y; d[u][2] = v.z; d[u][3] = v.w;
                }
            }
        }
        // scan_4<M>'s sum (query_common.hpp:72-80) in the grouping SM names
        float cand[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            float v[M];
#pragma unroll
            for (int b = 0; b < M / 2; ++b) {
                const uint32_t byte = (d[u][b >> 2] >> (8 * (b & 3))) & 0xffu;
                v[2 * b] = tab[(2 * b) * 16 + (byte & 15u)];
                v[2 * b + 1] = tab[(2 * b + 1) * 16 + (byte >> 4)];
            }
            cand[u] = adc_sum_code<M>(v, SM, 0.0f);
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (!live[u]) continue;
            if (it.filter) {
                // a value above the sample's R-th smallest cannot be the R-th smallest of the whole set
                if (!(cand[u] <= thr)) continue;
                const uint32_t ls = atomicAdd(&stage_n, 1u);
                if (ls < kStage) {
                    stage[ls] = cand[u];
                } else {                                     // staging full (rare): straight to the query's buffer
                    const uint32_t slot = base_n + atomicAdd(&qs->fc_n, 1u);
                    if (slot >= cap) { atomicOr(&qs->flags, 8u); continue; }
                    dst[slot] = cand[u];
                }
            } else {
                dst[it.out_off + i0 + u * stride] = cand[u];
            }
            const uint32_t k = fkey(cand[u]);
            kmin = min(kmin, k);
            kmax = max(kmax, k);
        }
    }
    // key range of the query's pre-scan values: lets the radix select skip the constant leading bits
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        kmin = min(kmin, (uint32_t)__shfl_xor(kmin, d, 64));
        kmax = max(kmax, (uint32_t)__shfl_xor(kmax, d, 64));
    }
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = kmin; red[4 + (threadIdx.x >> 6)] = kmax; }
    __syncthreads();
    const uint32_t ns = min(stage_n, (uint32_t)kStage);
    if (threadIdx.x == 0) {                                  // one atomic set per workgroup
        kmin = min(min(red[0], red[1]), min(red[2], red[3]));
        kmax = max(max(red[4], red[5]), max(red[6], red[7]));
        if (kmin <= kmax) {
            atomicMax(&qs->sel_nmin, ~kmin);
            atomicMax(&qs->sel_max, kmax);
        }
        if (ns) stage_base = base_n + atomicAdd(&qs->fc_n, ns);
    }
    __syncthreads();
    if (ns) {
        const uint32_t base = stage_base;
        for (uint32_t j = threadIdx.x; j < ns; j += 256) {
            if (base + j < cap) dst[base + j] = stage[j];
            else atomicOr(&qs->flags, 8u);
        }
    }
}

// Multi-query float pre-scan: the same sums for up to 8 queries in ONE pass over the starts (the float twin of
// scan_i8_mq_kernel).  LDS row (t, half, x) = { T_q[t][x] : q = 4*half .. 4*half+3 } = 16 bytes at
// t*512 + half*256 + x*16: two ds_read_b128 per code nibble, each conflict-free without replication (the 16 rows
// of a (t, half) block tile the 64 banks once; equal rows broadcast).  Every query's sum is grouped exactly as in
// the one-query kernel (SM: qadc_float_sum.h) — v_pk_add_f32 adds two queries per instruction with the rounding of
// v_add_f32 — so the values are bit-identical to that kernel's.  The as-compiled grouping is evaluated in a
// streaming order (pair sums as soon as both operands are loaded) so that at most six 8-query rows are live.
// Items of a group share codes / n / out_off / filter and differ in table / query.
typedef float fq_f32x4 __attribute__((ext_vector_type(4)));
struct FQ8 {                                                 // one value per query of the group
    fq_f32x4 lo, hi;
};
__device__ __forceinline__ FQ8 operator+(const FQ8& a, const FQ8& b) { return FQ8{a.lo + b.lo, a.hi + b.hi}; }
__device__ __forceinline__ FQ8 fq_row(uint32_t off) {
    typedef const __attribute__((address_space(3))) fq_f32x4* lds_frow_t;
    const fq_f32x4 lo = *reinterpret_cast<lds_frow_t>(static_cast<uintptr_t>(off));
    const fq_f32x4 hi = *reinterpret_cast<lds_frow_t>(static_cast<uintptr_t>(off + 256));
    return FQ8{lo, hi};
}
template <int M, int SM>
__global__ __launch_bounds__(256) void start_scan_mq_kernel(const StartItem* __restrict__ items, int nitems,
                                                            const float* __restrict__ ftables, float* __restrict__ fc,
                                                            uint64_t fc_stride, const uint32_t* __restrict__ fc_init,
                                                            QueryState* __restrict__ qstates) {
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    constexpr int kStageQ = 512;                             // survivors staged in LDS per query and workgroup
    constexpr int TAB = M * 512;
    float* stage = reinterpret_cast<float*>(smem + TAB);                 // [8][kStageQ]
    uint32_t* stage_n = reinterpret_cast<uint32_t*>(smem + TAB + kMQ * kStageQ * 4);   // [8]
    uint32_t* stage_base = stage_n + kMQ;                                              // [8]
    float* red = reinterpret_cast<float*>(stage_base + kMQ);                            // [2][8][4 waves]
    const int first_item = (int)blockIdx.y * kMQ;
    const int nq = min(kMQ, nitems - first_item);
    const StartItem* __restrict__ its = items + first_item;
    const StartItem it = its[0];
    const uint32_t tid = threadIdx.x;
    lds_base_is_zero();
    if (tid < kMQ) stage_n[tid] = 0;
    for (int e = tid; e < M * 16; e += 256) {                // e = t*16 + x
        float row[kMQ];
#pragma unroll
        for (int j = 0; j < kMQ; ++j) row[j] = j < nq ? ftables[(uint64_t)its[j].table * (M * 16) + e] : 0.0f;
        const int t = e >> 4, x = e & 15;
        *reinterpret_cast<f32x4*>(smem + t * 512 + x * 16) = f32x4{row[0], row[1], row[2], row[3]};
        *reinterpret_cast<f32x4*>(smem + t * 512 + 256 + x * 16) = f32x4{row[4], row[5], row[6], row[7]};
    }
    __syncthreads();
    // per query: destination, threshold (phase B), sample size and capacity; absent queries never store
    float thr[kMQ];
#pragma unroll
    for (int j = 0; j < kMQ; ++j) thr[j] = (j < nq && it.filter) ? qstates[its[j].query].qmax : 0.0f;
    constexpr int DW = M / 8;
    const uint32_t nib_mask = 0xf0u;
    float vmin[kMQ], vmax[kMQ];
#pragma unroll
    for (int j = 0; j < kMQ; ++j) { vmin[j] = FLT_MAX; vmax[j] = -FLT_MAX; }
    const uint32_t stride = gridDim.x * 256;
    for (uint32_t i = blockIdx.x * 256 + tid; i < it.n; i += stride) {
        uint32_t d[DW];
        if constexpr (M == 16) {
            typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
            const u32x2 v = ((const __attribute__((address_space(1))) u32x2*)(uintptr_t)it.codes)[i];
            d[0] = v.x; d[1] = v.y;
        } else {
            const u32x4_t v = ((const __attribute__((address_space(1))) u32x4_t*)(uintptr_t)it.codes)[i];
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        }
        // scan_4<M>'s sum (query_common.hpp:72-80) for the 8 queries at once, in the grouping SM names
#define QADC_FQ_L(w, k) fq_row(byte_and<(k)>(d[w] << 4, nib_mask) + (2 * (4 * (w) + (k))) * 512)
#define QADC_FQ_H(w, k) fq_row(byte_and<(k)>(d[w], nib_mask) + (2 * (4 * (w) + (k)) + 1) * 512)
        FQ8 s8;
        if constexpr (SM == 0) {
            s8 = FQ8{f32x4{0.0f, 0.0f, 0.0f, 0.0f}, f32x4{0.0f, 0.0f, 0.0f, 0.0f}};
#define QADC_FQ_BYTE(w, k) s8 = s8 + QADC_FQ_L(w, k); s8 = s8 + QADC_FQ_H(w, k);
#define QADC_FQ_WORD(w) QADC_FQ_BYTE(w, 0) QADC_FQ_BYTE(w, 1) QADC_FQ_BYTE(w, 2) QADC_FQ_BYTE(w, 3)
            QADC_FQ_WORD(0) QADC_FQ_WORD(1)
            if constexpr (M == 32) { QADC_FQ_WORD(2) QADC_FQ_WORD(3) }
#undef QADC_FQ_WORD
#undef QADC_FQ_BYTE
        } else {
            // A = (H2+L3)+(H3+L4), B = (H0+L1)+(H1+L2), C = (H5+L6)+(H4+L5), D = (H6+L7)+(H7+L0); s = ((A+B)+C)+D
            const FQ8 l0 = QADC_FQ_L(0, 0);
            FQ8 hp = QADC_FQ_H(0, 0);
            const FQ8 p0 = hp + QADC_FQ_L(0, 1); hp = QADC_FQ_H(0, 1);
            const FQ8 p1 = hp + QADC_FQ_L(0, 2); hp = QADC_FQ_H(0, 2);
            const FQ8 qb = p0 + p1;
            const FQ8 p2 = hp + QADC_FQ_L(0, 3); hp = QADC_FQ_H(0, 3);
            const FQ8 p3 = hp + QADC_FQ_L(1, 0); hp = QADC_FQ_H(1, 0);
            s8 = (p2 + p3) + qb;
            const FQ8 p4 = hp + QADC_FQ_L(1, 1); hp = QADC_FQ_H(1, 1);
            const FQ8 p5 = hp + QADC_FQ_L(1, 2); hp = QADC_FQ_H(1, 2);
            s8 = s8 + (p5 + p4);
            const FQ8 p6 = hp + QADC_FQ_L(1, 3); hp = QADC_FQ_H(1, 3);
            const FQ8 p7 = hp + l0;
            s8 = s8 + (p6 + p7);
            if constexpr (M == 32) {
                // s = s + ((L_{b+1}+H_{b+1}) + (L_b+H_b)), b = 8, 10, 12, 14
#define QADC_FQ_PAIR(w, k) s8 = s8 + ((QADC_FQ_L(w, (k) + 1) + QADC_FQ_H(w, (k) + 1)) + (QADC_FQ_L(w, k) + QADC_FQ_H(w, k)));
                QADC_FQ_PAIR(2, 0) QADC_FQ_PAIR(2, 2) QADC_FQ_PAIR(3, 0) QADC_FQ_PAIR(3, 2)
#undef QADC_FQ_PAIR
            }
        }
#undef QADC_FQ_L
#undef QADC_FQ_H
        const float cand[kMQ] = {s8.lo.x, s8.lo.y, s8.lo.z, s8.lo.w, s8.hi.x, s8.hi.y, s8.hi.z, s8.hi.w};
        if (!it.filter) {
#pragma unroll
            for (int j = 0; j < kMQ; ++j) {
                if (j >= nq) continue;
                fc[(uint64_t)its[j].query * fc_stride + it.out_off + i] = cand[j];
                const float rv = qadc_prescan_rank_value(cand[j]);   // (the key range is that of the rank images: fkey)
                vmin[j] = fminf(vmin[j], rv);
                vmax[j] = fmaxf(vmax[j], rv);
            }
        } else {
            bool any = false;
#pragma unroll
            for (int j = 0; j < kMQ; ++j) any |= (j < nq) && (cand[j] <= thr[j]);
            if (__builtin_expect(any, 0)) {
                // a value above the sample's R-th smallest cannot be the R-th smallest of the whole set
#pragma unroll
                for (int j = 0; j < kMQ; ++j) {
                    if (j >= nq || !(cand[j] <= thr[j])) continue;
                    vmin[j] = fminf(vmin[j], cand[j]);               // (cand <= thr <= FLT_MAX: its own rank image)
                    vmax[j] = fmaxf(vmax[j], cand[j]);
                    const uint32_t ls = atomicAdd(&stage_n[j], 1u);
                    if (ls < (uint32_t)kStageQ) {
                        stage[j * kStageQ + ls] = cand[j];
                    } else {                                 // staging full (rare): straight to the query's buffer
                        QueryState* qs = qstates + its[j].query;
                        const uint32_t base_n = fc_init[2 * its[j].query], cap = fc_init[2 * its[j].query + 1];
                        const uint32_t slot = base_n + atomicAdd(&qs->fc_n, 1u);
                        if (slot >= cap) { atomicOr(&qs->flags, 8u); continue; }
                        fc[(uint64_t)its[j].query * fc_stride + slot] = cand[j];
                    }
                }
            }
        }
    }
    // key range of each query's values (float order == key order; a sum accumulated from +0 is never -0)
#pragma unroll
    for (int j = 0; j < kMQ; ++j) {
#pragma unroll
        for (int dd = 32; dd >= 1; dd >>= 1) {
            vmin[j] = fminf(vmin[j], __shfl_xor(vmin[j], dd, 64));
            vmax[j] = fmaxf(vmax[j], __shfl_xor(vmax[j], dd, 64));
        }
        if ((tid & 63) == 0) { red[j * 4 + (tid >> 6)] = vmin[j]; red[32 + j * 4 + (tid >> 6)] = vmax[j]; }
    }
    __syncthreads();
    if (tid < (uint32_t)nq) {                                // one atomic set per workgroup and query
        const int j = (int)tid;
        const float mn = fminf(fminf(red[j * 4], red[j * 4 + 1]), fminf(red[j * 4 + 2], red[j * 4 + 3]));
        const float mx = fmaxf(fmaxf(red[32 + j * 4], red[32 + j * 4 + 1]), fmaxf(red[32 + j * 4 + 2], red[32 + j * 4 + 3]));
        QueryState* qs = qstates + its[j].query;
        if (mn <= mx) {
            atomicMax(&qs->sel_nmin, ~fkey(mn));
            atomicMax(&qs->sel_max, fkey(mx));
        }
        const uint32_t ns = min(stage_n[j], (uint32_t)kStageQ);
        if (ns) stage_base[j] = fc_init[2 * its[j].query] + atomicAdd(&qs->fc_n, ns);
    }
    __syncthreads();
    for (int j = 0; j < nq; ++j) {
        const uint32_t ns = min(stage_n[j], (uint32_t)kStageQ);
        if (!ns) continue;
        QueryState* qs = qstates + its[j].query;
        const uint32_t base = stage_base[j], cap = fc_init[2 * its[j].query + 1];
        for (uint32_t k = tid; k < ns; k += 256) {
            if (base + k < cap) fc[(uint64_t)its[j].query * fc_stride + base + k] = stage[j * kStageQ + k];
            else atomicOr(&qs->flags, 8u);
        }
    }
}

// groups of up to 8 consecutive items share codes / n / out_off / filter (the planner guarantees it)
void launch_start_scan_mq(int M, int sum_mode, const StartItem* d_items, int nitems, int wgs_per_group, const float* d_ftables, float* d_fc,
                          uint64_t fc_stride, const uint32_t* d_fc_init, QueryState* d_qs, hipStream_t stream) {
    const dim3 grid(wgs_per_group, (nitems + kMQ - 1) / kMQ), block(256);
    const size_t lds = (size_t)M * 512 + kMQ * 512 * 4 + 2 * kMQ * 4 + 64 * 4;
#define QADC_SSM(MM, SS) hipLaunchKernelGGL((start_scan_mq_kernel<MM, SS>), grid, block, lds, stream, d_items, nitems, d_ftables, d_fc, fc_stride, d_fc_init, d_qs)
    if (M == 16) { if (sum_mode) QADC_SSM(16, 1); else QADC_SSM(16, 0); }
    else         { if (sum_mode) QADC_SSM(32, 1); else QADC_SSM(32, 0); }
#undef QADC_SSM
}

// Exact float-ADC nearest code of a partition (smallest distance, lowest position on ties):
// the ground truth Recall@R is measured against when float ground truth over the raw vectors is
// not available.  Same sum as scan_4<M>, in the grouping sum_mode names (qadc_float_sum.h).
template <int M>
__global__ __launch_bounds__(256) void float_top1_kernel(const uint8_t* __restrict__ codes, uint32_t n,
                                                         const float* __restrict__ ftable, float* __restrict__ out_val,
                                                         uint32_t* __restrict__ out_pos, int sum_mode) {
    __shared__ float tab[M * 16];
    __shared__ float rv[256];
    __shared__ uint32_t rp[256];
    for (int i = threadIdx.x; i < M * 16; i += 256) tab[i] = ftable[i];
    __syncthreads();
    constexpr int DW = M / 8;
    float best = FLT_MAX;
    uint32_t bpos = 0xffffffffu;
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        uint32_t d[DW];
        if constexpr (M == 16) {
            const uint2 v = reinterpret_cast<const uint2*>(codes)[i];
            d[0] = v.x; d[1] = v.y;
        } else {
            const uint4 v = reinterpret_cast<const uint4*>(codes)[i];
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        }
        float v[M];
#pragma unroll
        for (int b = 0; b < M / 2; ++b) {
            const uint32_t byte = (d[b >> 2] >> (8 * (b & 3))) & 0xffu;
            v[2 * b] = tab[(2 * b) * 16 + (byte & 15u)];
            v[2 * b + 1] = tab[(2 * b + 1) * 16 + (byte >> 4)];
        }
        const float cand = adc_sum_code<M>(v, sum_mode, 0.0f);
        if (cand < best) { best = cand; bpos = i; }   // i ascends per thread: first minimum kept
    }
    rv[threadIdx.x] = best;
    rp[threadIdx.x] = bpos;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (threadIdx.x < s) {
            const float ov = rv[threadIdx.x + s];
            const uint32_t op = rp[threadIdx.x + s];
            if (ov < rv[threadIdx.x] || (ov == rv[threadIdx.x] && op < rp[threadIdx.x])) {
                rv[threadIdx.x] = ov;
                rp[threadIdx.x] = op;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) { out_val[blockIdx.x] = rv[0]; out_pos[blockIdx.x] = rp[0]; }
}

void launch_float_top1(int M, int sum_mode, const uint8_t* d_codes, uint32_t n, const float* d_ftable, float* d_val, uint32_t* d_pos,
                       int blocks, hipStream_t stream) {
    if (M == 16) hipLaunchKernelGGL(float_top1_kernel<16>, dim3(blocks), dim3(256), 0, stream, d_codes, n, d_ftable, d_val, d_pos, sum_mode);
    else         hipLaunchKernelGGL(float_top1_kernel<32>, dim3(blocks), dim3(256), 0, stream, d_codes, n, d_ftable, d_val, d_pos, sum_mode);
}

void launch_start_scan_f32(int M, int sum_mode, const StartItem* d_items, int nitems, int wgs_per_item, const float* d_ftables,
                           float* d_fc, uint64_t fc_stride, const uint32_t* d_fc_init, QueryState* d_qs, hipStream_t stream) {
    const dim3 grid(wgs_per_item, nitems), block(256);
#define QADC_SSF(MM, SS) hipLaunchKernelGGL((start_scan_f32_kernel<MM, SS>), grid, block, 0, stream, d_items, d_ftables, d_fc, fc_stride, d_fc_init, d_qs)
    if (M == 16) { if (sum_mode) QADC_SSF(16, 1); else QADC_SSF(16, 0); }
    else         { if (sum_mode) QADC_SSF(32, 1); else QADC_SSF(32, 0); }
#undef QADC_SSF
}

// ---------------------------------------------------------------------------------------------
// R-th smallest float per query (= tmp_bh.max() after query_scan_start, db_query_4.cpp:259):
// 4-pass MSD radix select on the order-preserving u32 image of the floats.
// ---------------------------------------------------------------------------------------------
// MSD radix select, one workgroup per query, on k' = key - min(key): only the bits below the range's
// top bit vary, so the first 8-bit digit already spreads the values over the LDS histogram.
// max_passes < 4 stops early and returns the UPPER edge of the digit bin reached: an upper bound of the
// R-th smallest, good enough (and valid) as the survivor filter of the pre-scan's second phase.
// QuantizerMAX<int8_t> (db_query_4.cpp:37-71) + qmin / clamp glue of query_scan (258-274), run by the query's
// select workgroup once qmax is known.
// quant_mode 1 = as compiled by the reference's flags: scale = 127/(max-min), trunc((v-min)*scale);
// quant_mode 0 = source level: trunc((v-min)/delta), delta = (max-min)/127.
// Strict IEEE float ops (build uses -ffp-contract=off, no fast-math), so results equal a CPU
// evaluation of the same expressions.
template <int BT>
__device__ void quantize_query(int table_dim_all, float* __restrict__ tb, int8_t* __restrict__ qt, QueryState* qs,
                               float qmax, int quant_mode, float* red /* [BT] LDS */, uint8_t* __restrict__ plane_sel,
                               uint8_t* __restrict__ plane_sel5, uint8_t* __restrict__ nib_sel, uint8_t* __restrict__ bkt_sel,
                               uint8_t* __restrict__ bktw_sel) {
    const int t = threadIdx.x;
    float m = FLT_MAX;
    for (int i = t; i < table_dim_all; i += BT) m = qadc_min_keep_nan(m, tb[i]);
    red[t] = m;
    __syncthreads();
    for (int d = BT / 2; d >= 1; d >>= 1) {
        if (t < d) red[t] = qadc_min_keep_nan(red[t], red[t + d]);
        __syncthreads();
    }
    float qmin = red[0];
    if (qmin != qmin) qmin = qadc_min_element_compiled(tb, table_dim_all, red, t);   // a NaN entry: the build's own order decides
    uint32_t flags = 0;
    if (qmin < 0) { qmin = 0; flags |= 2u; }
    if ((double)qmax > 1e30) flags |= 1u;                       // (a double compare, as db_query_4.cpp:271: 1e30f itself is above 1e30)
    const float delta = (qmax - qmin) / 127;
    const float scale = 127.0f / (qmax - qmin);
    for (int i = t; i < table_dim_all; i += BT) {
        float v = tb[i];
        if ((flags & 2u) && v < 0) { v = 0; tb[i] = 0; }       // (the clamp runs only when qmin < 0: not under a NaN qmin)
        int8_t o;
        if (flags & 1u) o = 127;   // query is skipped by the host; emit nothing
        else o = qadc_quantize_entry(v, qmin, qmax, scale, delta, quant_mode);
        qt[i] = o;
    }
    if (plane_sel || plane_sel5 || nib_sel || bkt_sel || bktw_sel) {   // 16x4: the 6-, 5-plane, nibble and bucket forms' choices of each table
        __syncthreads();
        for (int i = t; i < table_dim_all / 256; i += BT) {
            if (plane_sel) plane_sel[i] = (uint8_t)plane_choice(qt + (size_t)i * 256);
            if (plane_sel5) {
                const uint32_t c5 = plane_choice5(qt + (size_t)i * 256);
                plane_sel5[2 * i] = (uint8_t)(c5 & 0xffu);
                plane_sel5[2 * i + 1] = (uint8_t)(c5 >> 8);
            }
            if (nib_sel) plane_choice_nib(qt + (size_t)i * 256, nib_sel + (size_t)i * kNibSelBytes);
            if (bkt_sel) plane_choice_bkt(qt + (size_t)i * 256, bkt_sel + (size_t)i * kBktSelBytes);
            if (bktw_sel) plane_choice_bktw(qt + (size_t)i * 256, bktw_sel + (size_t)i * kBktwSelBytes);
        }
    }
    if (t == 0) { qs->qmin = qmin; qs->flags |= flags; }   // keeps bit3 set by the pre-scan
}

// BT threads per workgroup: 1024 for the level path's few queries with many values each; 256 for a batch of many queries
// (the throughput front of a partition-major batch: a 16-wave workgroup would wait for half a CU beside the scans).
// front_out (optional): {flags & 3, qmin, qmax, 0} per query, the record scan_query_kernel's HEAD takes as front_in.
template <int BT>
__global__ __launch_bounds__(BT) void select_kth_kernel(const float* __restrict__ fc, uint64_t fc_stride,
                                                        const uint32_t* __restrict__ fc_init, uint32_t R,
                                                        QueryState* __restrict__ qstates, int max_passes,
                                                        float* __restrict__ ftables, int8_t* __restrict__ qtables,
                                                        int table_dim_all, int quant_mode,
                                                        float* __restrict__ export_vals,
                                                        uint32_t* __restrict__ export_flags, uint32_t* __restrict__ front_out,
                                                        uint8_t* __restrict__ plane_sel, uint8_t* __restrict__ plane_sel5,
                                                        uint8_t* __restrict__ nib_sel, uint8_t* __restrict__ bkt_sel,
                                                        uint8_t* __restrict__ bktw_sel) {
    __shared__ uint32_t hist[256];
    __shared__ uint32_t s_prefix, s_k, s_hi, s_cnt;
    __shared__ float red[BT];
    const int q = blockIdx.x, tid = threadIdx.x;
    QueryState* qs = qstates + q;
    auto publish_front = [&]() {                             // (after quantize_query: thread 0 wrote qmin / flags / qmax itself)
        if (front_out && tid == 0) {
            uint32_t* fo = front_out + 4 * (size_t)q;
            fo[0] = qs->flags & 3u;
            fo[1] = __float_as_uint(qs->qmin);
            fo[2] = __float_as_uint(qs->qmax);
            fo[3] = 0;
        }
    };
    const uint32_t n = min(fc_init[2 * q] + qs->fc_n, fc_init[2 * q + 1]);
    if (export_flags && tid == 0) export_flags[q] = qs->flags;
    if (n < R) {                                           // heap never fills: max() stays the FLT_MAX sentinel
        if (export_vals) {                                 // sharded pre-scan: all n values, padded with the sentinel
            for (uint32_t i = tid; i < R; i += BT)
                export_vals[(uint64_t)q * R + i] = i < n ? fc[(uint64_t)q * fc_stride + i] : FLT_MAX;
        }
        if (tid == 0) qs->qmax = FLT_MAX;
        if (qtables) quantize_query<BT>(table_dim_all, ftables + (uint64_t)q * table_dim_all, qtables + (uint64_t)q * table_dim_all,
                                        qs, FLT_MAX, quant_mode, red, plane_sel ? plane_sel + (size_t)q * (table_dim_all / 256) : nullptr,
                                        plane_sel5 ? plane_sel5 + 2 * (size_t)q * (table_dim_all / 256) : nullptr,
                                        nib_sel ? nib_sel + (size_t)kNibSelBytes * q * (table_dim_all / 256) : nullptr,
                                        bkt_sel ? bkt_sel + (size_t)kBktSelBytes * q * (table_dim_all / 256) : nullptr,
                                        bktw_sel ? bktw_sel + (size_t)kBktwSelBytes * q * (table_dim_all / 256) : nullptr);
        publish_front();
        return;
    }
    const uint32_t kmin = ~qs->sel_nmin, kmax = qs->sel_max;
    const uint32_t range = kmax >= kmin ? kmax - kmin : 0u;
    if (tid == 0) { s_prefix = 0; s_k = R; s_hi = range ? 32u - (uint32_t)__clz(range) : 0u; }
    __syncthreads();
    const float* __restrict__ src = fc + (uint64_t)q * fc_stride;
    for (int pass = 0; pass < max_passes; ++pass) {
        const uint32_t hi = s_hi, prefix = s_prefix, k = s_k;
        if (hi == 0) break;
        const uint32_t lo = hi > 8 ? hi - 8 : 0;
        const uint32_t dmask = (1u << (hi - lo)) - 1u;
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        // 8 independent loads per thread and iteration: the loop is latency-bound otherwise (one workgroup)
        for (uint32_t i0 = tid; i0 < n; i0 += 8 * BT) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const uint32_t i = i0 + u * BT;
                v[u] = i < n ? src[i] : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                if (i0 + u * BT >= n) continue;
                const uint32_t key = fkey(v[u]) - kmin;
                if (hi >= 32 || ((key ^ prefix) >> hi) == 0) atomicAdd(&hist[(key >> lo) & dmask], 1u);
            }
        }
        __syncthreads();
        if (tid < 64) {                                    // wave 0: 4 bins per lane, inclusive scan, pick the digit
            const uint32_t c0 = hist[4 * tid], c1 = hist[4 * tid + 1], c2 = hist[4 * tid + 2], c3 = hist[4 * tid + 3];
            const uint32_t mine = c0 + c1 + c2 + c3;
            const uint32_t incl = dpp_wave_incl_sum(mine);
            const uint32_t excl = incl - mine;
            if (incl >= k && excl < k) {                   // exactly one lane
                uint32_t run = excl, digit = 4 * tid;
                const uint32_t cs[4] = {c0, c1, c2, c3};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (run + cs[j] >= k) { digit = 4 * tid + j; break; }
                    run += cs[j];
                }
                s_prefix = prefix | (digit << lo);
                s_k = k - run;
                s_hi = lo;
            }
        }
        __syncthreads();
    }
    const uint32_t low = s_hi ? ((s_hi >= 32 ? 0u : (1u << s_hi)) - 1u) : 0u;       // undecided bits -> all ones
    const uint64_t key = (uint64_t)(s_prefix | low) + kmin;
    const float qmax = funkey(key > kmax ? kmax : (uint32_t)key);                  // never above the largest stored value
    if (tid == 0) qs->qmax = qmax;
    if (export_vals) {
        // the R smallest values as a multiset (needs the exact R-th smallest: max_passes = 4): every value below
        // qmax, then qmax itself as often as it takes — which of several equal values is dropped does not matter
        if (tid == 0) s_cnt = 0;
        __syncthreads();
        for (uint32_t i = tid; i < n; i += BT) {
            const float v = src[i];
            if (v < qmax) export_vals[(uint64_t)q * R + atomicAdd(&s_cnt, 1u)] = v;    // fewer than R such values
        }
        __syncthreads();
        for (uint32_t i = s_cnt + tid; i < R; i += BT) export_vals[(uint64_t)q * R + i] = qmax;
    }
    if (qtables) quantize_query<BT>(table_dim_all, ftables + (uint64_t)q * table_dim_all, qtables + (uint64_t)q * table_dim_all,
                                    qs, qmax, quant_mode, red, plane_sel ? plane_sel + (size_t)q * (table_dim_all / 256) : nullptr,
                                        plane_sel5 ? plane_sel5 + 2 * (size_t)q * (table_dim_all / 256) : nullptr,
                                        nib_sel ? nib_sel + (size_t)kNibSelBytes * q * (table_dim_all / 256) : nullptr,
                                        bkt_sel ? bkt_sel + (size_t)kBktSelBytes * q * (table_dim_all / 256) : nullptr,
                                        bktw_sel ? bktw_sel + (size_t)kBktwSelBytes * q * (table_dim_all / 256) : nullptr);
    publish_front();
}

// Sharded pre-scan, second half: the gathered smallest values of all ranks stand in for the pre-scan output of
// a query.  One workgroup per query records their key range (what start_scan_f32_kernel does for its own values).
__global__ __launch_bounds__(256) void prescan_minmax_kernel(const float* __restrict__ vals, uint32_t nvals,
                                                             QueryState* __restrict__ qstates) {
    __shared__ uint32_t rmin[4], rmax[4];
    const int q = blockIdx.x, tid = threadIdx.x;
    uint32_t kmin = 0xffffffffu, kmax = 0;
    for (uint32_t i = tid; i < nvals; i += 256) {
        const uint32_t k = fkey(vals[(uint64_t)q * nvals + i]);
        kmin = min(kmin, k);
        kmax = max(kmax, k);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        kmin = min(kmin, (uint32_t)__shfl_xor(kmin, d, 64));
        kmax = max(kmax, (uint32_t)__shfl_xor(kmax, d, 64));
    }
    if ((tid & 63) == 0) { rmin[tid >> 6] = kmin; rmax[tid >> 6] = kmax; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w) { kmin = min(kmin, rmin[w]); kmax = max(kmax, rmax[w]); }
        qstates[q].sel_nmin = ~kmin;
        qstates[q].sel_max = kmax;
    }
}

void launch_prescan_minmax(const float* d_vals, uint32_t nvals, int nq, QueryState* d_qs, hipStream_t stream) {
    hipLaunchKernelGGL(prescan_minmax_kernel, dim3(nq), dim3(256), 0, stream, d_vals, nvals, d_qs);
}

void launch_select_kth(const float* d_fc, uint64_t fc_stride, const uint32_t* d_fc_init, int nq, uint32_t R, QueryState* d_qs,
                       int max_passes, float* d_ftables, int8_t* d_qtables, int table_dim_all, int quant_mode,
                       hipStream_t stream, float* export_vals, uint32_t* export_flags, uint32_t* d_front_out, int small_wg,
                       uint8_t* d_plane_sel, uint8_t* d_plane_sel5, uint8_t* d_nib_sel, uint8_t* d_bkt_sel,
                       uint8_t* d_bktw_sel) {
    if (small_wg)
        hipLaunchKernelGGL((select_kth_kernel<256>), dim3(nq), dim3(256), 0, stream, d_fc, fc_stride, d_fc_init, R, d_qs, max_passes,
                           d_ftables, d_qtables, table_dim_all, quant_mode, export_vals, export_flags, d_front_out, d_plane_sel,
                           d_plane_sel5, d_nib_sel, d_bkt_sel, d_bktw_sel);
    else
        hipLaunchKernelGGL((select_kth_kernel<1024>), dim3(nq), dim3(1024), 0, stream, d_fc, fc_stride, d_fc_init, R, d_qs, max_passes,
                           d_ftables, d_qtables, table_dim_all, quant_mode, export_vals, export_flags, d_front_out, d_plane_sel,
                           d_plane_sel5, d_nib_sel, d_bkt_sel, d_bktw_sel);
}

// ---- stream-layout probe (qadc_stream_probe): does a dispatch that WAITS FOR CUs on stream A hold up stream B? ----
// probe_spin_kernel: many 256-thread workgroups that hold 64 KiB of LDS each (two per CU: most wave slots stay free) and spin
// for spin_ticks of the 100 MHz wall clock: the launch keeps its queue's dispatcher waiting for CUs for several rounds.
// t[0] = first workgroup's start, t[1] = last workgroup's end, t[2] = start of probe_mark_kernel (launched on B right after).
__global__ __launch_bounds__(256) void probe_spin_kernel(unsigned long long* __restrict__ t, uint32_t spin_ticks) {
    extern __shared__ __attribute__((aligned(16))) unsigned char probe_lds[];
    const unsigned long long t0 = wall_clock64();
    if (threadIdx.x == 0) {
        probe_lds[0] = 1;
        atomicMin(&t[0], t0);
    }
    while (wall_clock64() - t0 < spin_ticks) __builtin_amdgcn_s_sleep(8);
    if (threadIdx.x == 0) atomicMax(&t[1], wall_clock64());
}
__global__ void probe_mark_kernel(unsigned long long* __restrict__ t) {
    if (threadIdx.x == 0) t[2] = wall_clock64();
}
hipError_t launch_stream_probe(unsigned long long* d_t, int spin_wgs, uint32_t spin_ticks, hipStream_t a, hipStream_t b) {
    static std::atomic<int> opted{0};
    if (!opted.exchange(1)) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&probe_spin_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 65536);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(probe_spin_kernel, dim3(spin_wgs), dim3(256), 65536, a, d_t, spin_ticks);
    hipLaunchKernelGGL(probe_mark_kernel, dim3(1), dim3(64), 0, b, d_t);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Host feeders on the device: coarse assignment, residuals, float distance tables.
// Plain sequential float arithmetic (no FMA contraction), so a host evaluation of the same loops
// (host/query_driver.hpp) gives identical bits.
// ---------------------------------------------------------------------------------------------
// ---- find_k_neighbors' selection WITH exact float ties (neighbors.cpp:18-28, 47-71; binheap.hpp:75-127) ----
// The select kernels below pick "the ma smallest by (distance, index)".  That IS what the reference's heaps leave whenever no two
// of the kept-or-boundary distances are exactly equal (pinned: tests/test_oracle_float_ref.py).  With exact ties the reference's
// result depends on its heap's history — a kv_binheap<int, float> of capacity ma takes the K distances in index order (push: a
// full heap accepts only values strictly below its root, the root sinks preferring the LEFT child on equal children) — and on the
// order std::sort leaves equal keys in (libstdc++ introsort on the permutation 0..ma-1 of the heap array, comparator
// value[a] < value[b]: median-of-3 quicksort loop down to ranges of 16, depth limit 2 floor(log2 n) with heapsort below it, one
// final insertion sort — GCC 11.4 bits/stl_algo.h, the same restatement as the oracle's sort_keys).  A select kernel that SEES a
// tie (two equal values among its ma, or a value equal to the ma-th outside them) calls this for its query: wave 0, the heap and
// the permutation in LDS, lane 0 doing the sequential part, the other lanes only the loads and the pre-filter (a chunk of 64
// distances none of which is below the root is skipped with one ballot).  ma <= 256.
struct ExactSel {
    float* hv;      // [256] heap values
    int* hk;        // [256] heap keys
    int* perm;      // [256] permutation sorted by std::sort's algorithm; then [72]: the quicksort loop's pending ranges
};
constexpr int kExactSelInts = 256 + 72;     // (everything lives in LDS: a private array would give the select kernels a scratch segment)

__device__ __forceinline__ bool xs_less(const ExactSel& x, int a, int b) { return x.hv[a] < x.hv[b]; }

__device__ __forceinline__ void xs_push_heap(const ExactSel& x, int* first, int hole, int top, int value) {      // std::__push_heap
    int parent = (hole - 1) / 2;
    while (hole > top && xs_less(x, first[parent], value)) {
        first[hole] = first[parent];
        hole = parent;
        parent = (hole - 1) / 2;
    }
    first[hole] = value;
}

__device__ __forceinline__ void xs_adjust_heap(const ExactSel& x, int* first, int hole, int len, int value) {    // std::__adjust_heap
    const int top = hole;
    int child = hole;
    while (child < (len - 1) / 2) {
        child = 2 * (child + 1);
        if (xs_less(x, first[child], first[child - 1])) child--;
        first[hole] = first[child];
        hole = child;
    }
    if ((len & 1) == 0 && child == (len - 2) / 2) {
        child = 2 * (child + 1);
        first[hole] = first[child - 1];
        hole = child - 1;
    }
    xs_push_heap(x, first, hole, top, value);
}

__device__ __forceinline__ void xs_heapsort(const ExactSel& x, int* first, int* last) {                          // std::__partial_sort(first, last, last)
    const int len = (int)(last - first);
    if (len >= 2)
        for (int parent = (len - 2) / 2;; --parent) {
            xs_adjust_heap(x, first, parent, len, first[parent]);
            if (parent == 0) break;
        }
    while (last - first > 1) {
        --last;
        const int value = *last;
        *last = *first;
        xs_adjust_heap(x, first, 0, (int)(last - first), value);
    }
}

__device__ __forceinline__ void xs_linear_insert(const ExactSel& x, int* last) {                                 // std::__unguarded_linear_insert
    const int val = *last;
    int* next = last - 1;
    while (xs_less(x, val, *next)) {
        *last = *next;
        last = next;
        --next;
    }
    *last = val;
}

__device__ __forceinline__ void xs_insertion_sort(const ExactSel& x, int* first, int* last) {                    // std::__insertion_sort
    if (first == last) return;
    for (int* i = first + 1; i != last; ++i) {
        if (xs_less(x, *i, *first)) {
            const int val = *i;
            for (int* p = i; p != first; --p) *p = *(p - 1);                                      // std::move_backward
            *first = val;
        } else {
            xs_linear_insert(x, i);
        }
    }
}

__device__ __forceinline__ void xs_std_sort(const ExactSel& x, int n) {
    int* perm = x.perm;
    int lg = 0;
    for (int m = n; m > 1; m >>= 1) ++lg;
    // std::__introsort_loop, its tail recursion on [cut, last) as an explicit stack (at most 2 lg + 1 ranges deep)
    int* st_first = x.perm + 256; int* st_last = st_first + 24; int* st_depth = st_last + 24;
    int sp = 0;
    st_first[0] = 0; st_last[0] = n; st_depth[0] = 2 * lg; sp = 1;
    while (sp > 0) {
        --sp;
        int first = st_first[sp], last = st_last[sp], depth = st_depth[sp];
        // (the recursion handles [cut, last) FIRST and then continues with [first, cut): ranges are disjoint, so the order in which
        // they are processed does not change the result; here the right part is stacked and the left one continues)
        while (last - first > 16) {
            if (depth == 0) {
                xs_heapsort(x, perm + first, perm + last);
                break;
            }
            --depth;
            const int mid = first + (last - first) / 2;
            {                                                                                     // std::__move_median_to_first(first, first + 1, mid, last - 1)
                int* r = perm + first; int* a = perm + first + 1; int* b = perm + mid; int* c = perm + last - 1;
                int* pick;
                if (xs_less(x, *a, *b)) pick = xs_less(x, *b, *c) ? b : (xs_less(x, *a, *c) ? c : a);
                else pick = xs_less(x, *a, *c) ? a : (xs_less(x, *b, *c) ? c : b);
                const int t = *r; *r = *pick; *pick = t;
            }
            int lo = first + 1, hi = last;                                                       // std::__unguarded_partition(first + 1, last, first)
            for (;;) {
                while (xs_less(x, perm[lo], perm[first])) ++lo;
                --hi;
                while (xs_less(x, perm[first], perm[hi])) --hi;
                if (!(lo < hi)) break;
                const int t = perm[lo]; perm[lo] = perm[hi]; perm[hi] = t;
                ++lo;
            }
            if (sp < 24) { st_first[sp] = lo; st_last[sp] = last; st_depth[sp] = depth; ++sp; }
            last = lo;
        }
    }
    if (n > 16) {                                                                                 // std::__final_insertion_sort
        xs_insertion_sort(x, perm, perm + 16);
        for (int* i = perm + 16; i != perm + n; ++i) xs_linear_insert(x, i);
    } else {
        xs_insertion_sort(x, perm, perm + n);
    }
}

// Rows with a NaN distance (any query: one workgroup's barrier-wide OR; uniform result).  NaN breaks the (distance, index) order
// the fast selections rest on — the reference's compiled heap lets a NaN replace the top (coarse_exact_select) — so such a row is
// replayed exactly.  The replay's heap lives in LDS arrays of 256: a NaN row with ma > 256 is counted in g_coarse_nan_unreplayed
// instead (its assign[] still holds indices in [0, K)), and the entry points that read the counter fail.
__device__ unsigned int g_coarse_nan_unreplayed;

__device__ __forceinline__ bool coarse_nan_row(int lane_nan, int ma) {
    const bool row = __syncthreads_or(lane_nan) != 0;
    if (row && ma > 256) {
        if (threadIdx.x == 0) atomicAdd(&g_coarse_nan_unreplayed, 1u);
        return false;
    }
    return row;
}

// Distances of either sign as unsigned keys that order like the values (positive: sign bit set; negative: all bits flipped; -0 does
// not occur: a sum of a non-negative and a product rounds to +0); 0xffffffff stays above every finite key: the padding past K.
__device__ __forceinline__ uint32_t coarse_key(float f) {
    const uint32_t b = __float_as_uint(f);
    return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}

// called by every lane of wave 0 (lane = 0..63); dq = the query's K distances in global memory.
// The comparisons are the reference's AS COMPILED (-ffast-math; read off its build, oracle/qadc_oracle.c orc_select_k_neighbors):
// sift-up v > parent, replace-top !(v >= top) — a NaN replaces the top and any value replaces a NaN top —, sift-down right > left
// and stop iff value >= largest, std::sort's v[a] < v[b].  The ballot pre-filter drops the values the top rejects; that holds for
// the rest of a 64-chunk only while the top cannot grow, i.e. until the first NaN of the row: from there on every value is pushed.
__device__ __forceinline__ void coarse_exact_select(const float* __restrict__ dq, int K, int ma, int32_t* __restrict__ out,
                                                 float* hv, int* hk, int* perm, uint32_t lane) {
    const ExactSel x{hv, hk, perm};
    int size = 0;
    bool seen_nan = false;
    for (int k0 = 0; k0 < K; k0 += 64) {
        const int k = k0 + (int)lane;
        const float v = k < K ? dq[k] : 0.0f;
        seen_nan = seen_nan || __builtin_amdgcn_ballot_w64(k < K && v != v) != 0;                  // (uniform)
        uint64_t todo = __builtin_amdgcn_ballot_w64(k < K && (size < ma || seen_nan || !(v >= hv[0])));
        while (todo) {
            const int j = (int)__builtin_ctzll(todo);
            todo &= todo - 1;
            const float vj = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(v), j));
            if (lane == 0) {                                                                      // kv_binheap::push (binheap.hpp:75-116)
                if (size != ma) {
                    int i = size;
                    hv[i] = vj; hk[i] = k0 + j;
                    int parent = (i - 1) / 2;
                    while (i != 0 && hv[i] > hv[parent]) {
                        const float tv = hv[i]; hv[i] = hv[parent]; hv[parent] = tv;
                        const int tk = hk[i]; hk[i] = hk[parent]; hk[parent] = tk;
                        i = parent;
                        parent = (i - 1) / 2;
                    }
                } else if (!(vj >= hv[0])) {                                                      // (vcomiss + jae)
                    int i = 0;
                    hv[0] = vj; hk[0] = k0 + j;
                    for (;;) {
                        const int l = 2 * i + 1, r = 2 * i + 2;
                        if (l >= ma) break;
                        int c = l;
                        if (r < ma && hv[r] > hv[l]) c = r;
                        if (hv[i] >= hv[c]) break;                                                // (vcomiss + jb)
                        const float tv = hv[i]; hv[i] = hv[c]; hv[c] = tv;
                        const int tk = hk[i]; hk[i] = hk[c]; hk[c] = tk;
                        i = c;
                    }
                }
            }
            if (size != ma) ++size;                                                               // (uniform: every lane counts)
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    for (int i = (int)lane; i < size; i += 64) perm[i] = i;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) xs_std_sort(x, size);                                                          // kv_binheap::sort (binheap.hpp:118-127)
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (int i = (int)lane; i < size; i += 64) out[i] = hk[perm[i]];
}

// KPT = centroids per thread kept in registers (K <= 256 * KPT); KPT == 0: distances live in the global scratch.
// Every thread accumulates ITS centroid's dimensions in ascending order (bit-exact with the host loop); a
// thread walks one row sequentially, so each cache line it touches is reused 16 times from L1 and the K x dim
// matrix (shared by every query's workgroup) stays in L2.
// QB = queries per workgroup: a thread walks ITS centroid rows once and accumulates the QB queries' distances side by
// side (each in its own ascending-d order, so every sum is bit-exact with the host loop) — the K x dim matrix is read
// nq/QB times instead of nq times, which is what this kernel is bound by.
// ||row||^2 of n rows of `dim` floats, one thread per row, in the grouping the reference's compute_cross_dists_blas adds it
// (fmanorm<dim/8, dim%8> as compiled; expansion_sqnorm): the ||q||^2 and ||c||^2 of the coarse distances below.
__global__ __launch_bounds__(256) void row_sqnorm_kernel(const float* __restrict__ rows, int n, int dim, int sum_mode, float* __restrict__ out) {
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i < n) out[i] = expansion_sqnorm(rows + (size_t)i * dim, dim, sum_mode);
}

// The coarse distances are the reference's: find_k_neighbors (neighbors.cpp:30-76) takes them from compute_cross_dists_blas<dim>
// (distances.hpp:151-183): (||q||^2 + ||c||^2) — qnorm / cnorm, as compiled — then sgemm(alpha = -2, beta = 1) adds -2 q.c; the
// product is restated as ONE sequential dot in ascending d (OpenBLAS is not in this image), the sum rounds once.  They can come
// out slightly negative for q ~ c: the selections below order floats of either sign.
template <int KPT, int QB>
__global__ __launch_bounds__(256) void coarse_assign_kernel(const float* __restrict__ queries,
                                                            const float* __restrict__ coarse, int nq, int K, int dim, int ma,
                                                            const float* __restrict__ qnorm, const float* __restrict__ cnorm,
                                                            float* __restrict__ dist, int32_t* __restrict__ assign) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
    float* q = reinterpret_cast<float*>(dyn);                 // [QB][dim]
    __shared__ uint32_t rv[4], rk[4];
    const int q0 = blockIdx.x * QB, tid = threadIdx.x;
    const int nqb = min(QB, nq - q0);
    for (int i = tid; i < QB * dim; i += 256) {
        const int b = i / dim, d = i - b * dim;
        q[i] = b < nqb ? queries[(size_t)(q0 + b) * dim + d] : 0.0f;
    }
    __syncthreads();
    constexpr int NR = KPT > 0 ? KPT : 1;
    float mine[NR][QB];
    int nan[QB];
#pragma unroll
    for (int b = 0; b < QB; ++b) nan[b] = 0;
#pragma unroll
    for (int j = 0; j < NR; ++j)
#pragma unroll
        for (int b = 0; b < QB; ++b) mine[j][b] = FLT_MAX;
    const int nblk = (K + 255) / 256;
    auto row_dist = [&](int k, float (&s)[QB]) {
        const float* __restrict__ c = coarse + (size_t)k * dim;
#pragma unroll
        for (int b = 0; b < QB; ++b) s[b] = 0.0f;
        for (int d = 0; d < dim; ++d) {
            const float cv = c[d];
#pragma unroll
            for (int b = 0; b < QB; ++b) s[b] += q[b * dim + d] * cv;
        }
        const float cn = cnorm[k];
#pragma unroll
        for (int b = 0; b < QB; ++b) s[b] = (qnorm[min(q0 + b, nq - 1)] + cn) + (-2.0f * s[b]);
    };
    if (KPT > 0) {
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            const int k = j * 256 + tid;
            if (j < nblk && k < K) {
                row_dist(k, mine[j]);
#pragma unroll
                for (int b = 0; b < QB; ++b) nan[b] |= mine[j][b] != mine[j][b];
                if (dist)                                        // (the exact-tie path below reads the row from memory)
#pragma unroll
                    for (int b = 0; b < QB; ++b)
                        if (b < nqb) dist[(size_t)(q0 + b) * K + k] = mine[j][b];
            }
        }
    } else {
        for (int k = tid; k < K; k += 256) {
            float s[QB];
            row_dist(k, s);
#pragma unroll
            for (int b = 0; b < QB; ++b) {
                nan[b] |= s[b] != s[b];
                if (b < nqb) dist[(size_t)(q0 + b) * K + k] = s[b];
            }
        }
    }
    __syncthreads();
    __shared__ float x_hv[256];
    __shared__ int x_hk[256], x_perm[kExactSelInts];
    // per query: ma rounds of "smallest (key, index) strictly after the previous pick" in coarse_key's order (+ one more round
    // that only looks for a value equal to the ma-th outside the picks: an exact tie, see coarse_exact_select).  Keys, not
    // floats: +inf and FLT_MAX are ordinary candidates, and (0xffffffff, 0xffffffff) is beaten by every (key, k < K), so
    // with ma <= K every pick is an index in [0, K).  A row with a NaN is replayed exactly afterwards (coarse_nan_row).
#pragma unroll
    for (int b = 0; b < QB; ++b) {
        if (b >= nqb) break;
        const float* __restrict__ dq = dist + (size_t)(q0 + b) * K;
        uint32_t last_v = 0;
        int last_k = -1;
        bool tie = false;
        const int rounds = (dist && ma > 1 && ma <= 256 && ma < K) ? ma + 1 : ma;
        for (int a = 0; a < rounds; ++a) {
            uint32_t bv = 0xffffffffu, bk = 0xffffffffu;
            if (KPT > 0) {
#pragma unroll
                for (int j = 0; j < NR; ++j) {
                    const int k = j * 256 + tid;
                    const uint32_t v = coarse_key(mine[j][b]);
                    const bool after = v > last_v || (v == last_v && k > last_k);
                    if (k < K && after && (v < bv || (v == bv && (uint32_t)k < bk))) { bv = v; bk = (uint32_t)k; }
                }
            } else {
                for (int k = tid; k < K; k += 256) {
                    const uint32_t v = coarse_key(dq[k]);
                    const bool after = v > last_v || (v == last_v && k > last_k);
                    if (after && (v < bv || (v == bv && (uint32_t)k < bk))) { bv = v; bk = (uint32_t)k; }
                }
            }
            // wave-level reduction first (no barrier), then across the 4 waves through LDS
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                const uint32_t ov = __shfl_xor(bv, d, 64);
                const uint32_t ok = __shfl_xor(bk, d, 64);
                if (ov < bv || (ov == bv && ok < bk)) { bv = ov; bk = ok; }
            }
            if ((tid & 63) == 0) { rv[tid >> 6] = bv; rk[tid >> 6] = bk; }
            __syncthreads();
            bv = rv[0];
            bk = rk[0];
#pragma unroll
            for (int w = 1; w < 4; ++w)
                if (rv[w] < bv || (rv[w] == bv && rk[w] < bk)) { bv = rv[w]; bk = rk[w]; }
            tie = tie || (a > 0 && bv == last_v && bk != 0xffffffffu);
            last_v = bv;
            last_k = (int)bk;
            if (tid == 0 && a < ma) assign[(size_t)(q0 + b) * ma + a] = last_k;
            __syncthreads();
        }
        if (dist && coarse_nan_row(nan[b], ma)) tie = true;      // (a NaN row: the exact replay, as for a tie)
        if (tie && dist && ma <= 256) {                          // (uniform: every thread saw the same picks)
            __threadfence_block();
            if (tid < 64) coarse_exact_select(dq, K, ma, assign + (size_t)(q0 + b) * ma, x_hv, x_hk, x_perm, (uint32_t)tid);
            __syncthreads();
        }
    }
}

// ---- the same arithmetic as two lean kernels (what every batch with dim % 4 == 0 and K <= 16384 takes) ----
// coarse_assign_kernel keeps a query group's K distances in registers (64 accumulators per lane at K = 4096) and reads
// its centroid rows one row per lane.  Under the pipelined IVF batches that is the most expensive kernel of the front.
// Here (1) coarse_dist_kernel computes [16 queries] x [256 centroids] distance tiles — centroid tiles staged through LDS
// with 16-byte coalesced loads (the next tile's loads in flight), transposed so that lane k reads tile[d][k] without
// bank conflicts, the 16 queries' components as LDS broadcasts, 16 accumulators per lane — into the [nq][K] scratch,
// and (2) coarse_select_kernel picks the ma nearest per query.  Every (query, centroid) sum still accumulates
// d = 0, 1, 2 ... in order, and the selection applies the same (distance, index) order: same assign[] bit for bit.
constexpr int kCDQ = 16, kCDC = 32, kCDStride = 257;

__device__ __forceinline__ uint32_t dpp_wave_min_u32(uint32_t x) {
    uint32_t v = x;
    const int id = -1;                                           // 0xffffffff: identity of min
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(id, (int)x, 0x111, 0xf, 0xf, false));
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(id, (int)x, 0x112, 0xf, 0xf, false));
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(id, (int)x, 0x113, 0xf, 0xf, false));
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(id, (int)v, 0x114, 0xf, 0xe, false));
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(id, (int)v, 0x118, 0xf, 0xc, false));
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(id, (int)v, 0x142, 0xa, 0xf, false));
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(id, (int)v, 0x143, 0xc, 0xf, false));
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

__global__ __launch_bounds__(256) void coarse_dist_kernel(const float* __restrict__ queries, const float* __restrict__ coarse,
                                                          int nq, int K, int dim, const float* __restrict__ qnorm,
                                                          const float* __restrict__ cnorm, float* __restrict__ dist) {
    __shared__ float tile[kCDC * kCDStride];                     // [d][centroid]
    __shared__ __attribute__((aligned(16))) float qt[kCDC * kCDQ];   // [d][query]
    const int tid = threadIdx.x;
    const int k0 = blockIdx.x * 256, q0 = blockIdx.y * kCDQ;
    const int lrow = tid >> 3, lcol = (tid & 7) * 4;           // this thread's float4s of a tile: rows lrow + 32p, columns lcol..lcol+3
    float acc[kCDQ];
#pragma unroll
    for (int b = 0; b < kCDQ; ++b) acc[b] = 0.0f;
    float4 pre[8];
    float qpre[2];
    auto fetch = [&](int d0) {
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            const int k = k0 + lrow + 32 * p, d = d0 + lcol;
            pre[p] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (k < K && d < dim) pre[p] = *reinterpret_cast<const float4*>(coarse + (size_t)k * dim + d);   // (dim % 4 == 0)
        }
#pragma unroll
        for (int e = 0; e < 2; ++e) {                            // the query chunk [16][32]: element (b, dd) = tid + 256 e
            const int i = tid + 256 * e, b = i / kCDC, dd = i % kCDC;
            const int q = min(q0 + b, nq - 1), d = d0 + dd;      // (a ragged last group repeats its last query)
            qpre[e] = d < dim ? queries[(size_t)q * dim + d] : 0.0f;
        }
    };
    fetch(0);
    for (int d0 = 0; d0 < dim; d0 += kCDC) {
        const int dcn = min(kCDC, dim - d0);
        __syncthreads();                                         // the previous tile has been consumed
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            const int r = lrow + 32 * p;
            tile[(lcol + 0) * kCDStride + r] = pre[p].x;
            tile[(lcol + 1) * kCDStride + r] = pre[p].y;
            tile[(lcol + 2) * kCDStride + r] = pre[p].z;
            tile[(lcol + 3) * kCDStride + r] = pre[p].w;
        }
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int i = tid + 256 * e;
            qt[(i % kCDC) * kCDQ + i / kCDC] = qpre[e];
        }
        __syncthreads();
        if (d0 + kCDC < dim) fetch(d0 + kCDC);                   // in flight while this tile is consumed
        for (int dd = 0; dd < dcn; ++dd) {
            const float cv = tile[dd * kCDStride + tid];
            // two queries per instruction: v_pk_mul_f32 + v_pk_add_f32 — each component is the IEEE result of the scalar operation
            // (no contraction: -ffp-contract=off), the dots stay sequential in d
            typedef float f32x2 __attribute__((ext_vector_type(2)));
            const f32x2 cv2 = {cv, cv};
#pragma unroll
            for (int b4 = 0; b4 < kCDQ / 4; ++b4) {
                const float4 t4 = *reinterpret_cast<const float4*>(&qt[dd * kCDQ + 4 * b4]);   // same address in every lane: broadcast
                const f32x2 q01 = {t4.x, t4.y}, q23 = {t4.z, t4.w};
                const f32x2 s01 = q01 * cv2, s23 = q23 * cv2;
                acc[4 * b4] += s01.x; acc[4 * b4 + 1] += s01.y; acc[4 * b4 + 2] += s23.x; acc[4 * b4 + 3] += s23.y;
            }
        }
    }
    const int k = k0 + tid;
    if (k < K) {
        const float cn = cnorm[k];
#pragma unroll
        for (int b = 0; b < kCDQ; ++b)
            if (q0 + b < nq) dist[(size_t)(q0 + b) * K + k] = (qnorm[q0 + b] + cn) + (-2.0f * acc[b]);
    }
}

// ma rounds of "smallest (distance, index) strictly after the previous pick" over a query's K distances (as coarse_key);
// one workgroup per query, KPT distances per lane in registers
template <int KPT>
__global__ __launch_bounds__(256) void coarse_select_kernel(const float* __restrict__ dist, int K, int ma, int32_t* __restrict__ assign) {
    __shared__ uint32_t rv[2][4], rk[2][4];
    const int q = blockIdx.x, tid = threadIdx.x;
    uint32_t mine[KPT];
    int nan = 0;
#pragma unroll
    for (int j = 0; j < KPT; ++j) {
        const int k = j * 256 + tid;
        const float f = k < K ? dist[(size_t)q * K + k] : 0.0f;
        nan |= f != f;
        mine[j] = k < K ? coarse_key(f) : 0xffffffffu;
    }
    __shared__ float x_hv[256];
    __shared__ int x_hk[256], x_perm[kExactSelInts];
    if (coarse_nan_row(nan, ma)) {                               // a NaN: the reference's heap history decides (uniform branch)
        if (tid < 64) coarse_exact_select(dist + (size_t)q * K, K, ma, assign + (size_t)q * ma, x_hv, x_hk, x_perm, (uint32_t)tid);
        return;
    }
    uint32_t last_v = 0;
    int last_k = -1, par = 0;
    bool tie = false;
    const int rounds = (ma > 1 && ma <= 256 && ma < K) ? ma + 1 : ma;   // (the extra round looks for a value equal to the ma-th outside the picks)
    for (int a = 0; a < rounds; ++a, par ^= 1) {
        uint32_t bv = 0xffffffffu, bk = 0xffffffffu;
#pragma unroll
        for (int j = 0; j < KPT; ++j) {
            const uint32_t k = (uint32_t)(j * 256 + tid);
            const uint32_t v = mine[j];
            const bool after = v > last_v || (v == last_v && (int)k > last_k);
            if (k < (uint32_t)K && after && (v < bv || (v == bv && k < bk))) { bv = v; bk = k; }
        }
        const uint32_t wv = dpp_wave_min_u32(bv);
        const uint32_t wk = dpp_wave_min_u32(bv == wv ? bk : 0xffffffffu);
        if ((tid & 63) == 0) { rv[par][tid >> 6] = wv; rk[par][tid >> 6] = wk; }
        __syncthreads();                                         // (slots alternate: one barrier per round)
        bv = rv[par][0];
        bk = rk[par][0];
#pragma unroll
        for (int w = 1; w < 4; ++w)
            if (rv[par][w] < bv || (rv[par][w] == bv && rk[par][w] < bk)) { bv = rv[par][w]; bk = rk[par][w]; }
        tie = tie || (a > 0 && bv == last_v && bk != 0xffffffffu);
        last_v = bv;
        last_k = (int)bk;
        if (tid == 0 && a < ma) assign[(size_t)q * ma + a] = last_k;
    }
    if (tie && ma <= 256) {                                      // exact float ties: the reference's heap history decides (coarse_exact_select)
        __syncthreads();
        if (tid < 64) coarse_exact_select(dist + (size_t)q * K, K, ma, assign + (size_t)q * ma, x_hv, x_hk, x_perm, (uint32_t)tid);
    }
}

// The same selection for ma <= 256 without the ma dependent rounds: (1) the ma-th smallest key by a 4-pass MSD radix
// select over the K distances (8 bits per pass, 256-bin histogram in LDS); (2) every key below it, and the needed number
// of keys EQUAL to it with the smallest indices, collected into LDS; (3) one bitonic sort of those ma (key, index) pairs.
// Result identical to the rounds above (ascending distance, lower index first on ties); K = 16384, ma = 64: 330 -> ~25 us
// for a workgroup on its own, which is what a rank's share of a sharded front waits for.
// An exact float tie — a value equal to the ma-th outside the picks, or two equal values among them — hands the query to
// coarse_exact_select (the reference's heap history decides); without ties the result is the reference's entry for entry.
template <int KPT>
__global__ __launch_bounds__(256) void coarse_select_radix_kernel(const float* __restrict__ dist, int K, int ma, int32_t* __restrict__ assign) {
    __shared__ uint32_t hist[256];
    __shared__ __attribute__((aligned(16))) uint64_t cand[256];
    __shared__ uint32_t ties[256];
    __shared__ uint32_t s_prefix, s_rank, s_nless, s_nties, s_kept, s_T0;
    const int q = blockIdx.x, tid = threadIdx.x;
    __shared__ float x_hv[256];
    __shared__ int x_hk[256], x_perm[kExactSelInts];
    uint32_t mine[KPT];
    int nan = 0;
#pragma unroll
    for (int j = 0; j < KPT; ++j) {
        const int k = j * 256 + tid;
        const float f = k < K ? dist[(size_t)q * K + k] : 0.0f;
        nan |= f != f;
        mine[j] = k < K ? coarse_key(f) : 0xffffffffu;
    }
    if (coarse_nan_row(nan, ma)) {                               // a NaN: the reference's heap history decides (uniform branch)
        if (tid < 64) coarse_exact_select(dist + (size_t)q * K, K, ma, assign + (size_t)q * ma, x_hv, x_hk, x_perm, (uint32_t)tid);
        return;
    }
    if (tid == 0) { s_prefix = 0; s_rank = (uint32_t)ma; s_nless = 0; s_nties = 0; s_kept = 0; s_T0 = 0xffffffffu; }
    __syncthreads();
    // Threshold first (round 4, as in the query kernel's front select): ma is a percent or less of K, and counting ALL K
    // distances into digit bins is one LDS atomic per value on one or two hot bins — 16384 serialized adds per pass at the C5
    // shape.  Wave 0 ranks the first 64 distances (centroid order carries no distance order) and takes the m-th smallest,
    // m = 1.5 x the ma-th value's expected rank among 64, + 3; only distances <= that take part in the passes (a few
    // percent of K; the ma smallest are among them as long as at least ma are kept — counted; if not, no filter).
    if (tid < 64) {
        const uint32_t sk = mine[0];                             // (k = tid; 0xffffffff past K)
        const uint32_t m = min(64u, (uint32_t)((96ull * (uint32_t)ma + (uint32_t)K - 1u) / (uint32_t)K) + 3u);
        uint32_t less = 0, le = 0;
#pragma unroll 8
        for (int j = 0; j < 64; ++j) {
            const uint32_t kj = (uint32_t)__builtin_amdgcn_readlane((int)sk, j);
            less += kj < sk ? 1u : 0u;
            le += kj <= sk ? 1u : 0u;
        }
        if (less < m && m <= le) s_T0 = sk;
    }
    __syncthreads();
    uint32_t T0 = s_T0;
    {
        uint32_t c = 0;
#pragma unroll
        for (int j = 0; j < KPT; ++j) c += (j * 256 + tid < K && mine[j] <= T0) ? 1u : 0u;
        c = dpp_wave_incl_sum(c);
        if ((tid & 63) == 63) atomicAdd(&s_kept, c);
    }
    __syncthreads();
    if (s_kept < (uint32_t)ma) T0 = 0xffffffffu;                 // (an unlucky sample: everything takes part, as before)
    for (int pass = 3; pass >= 0; --pass) {
        hist[tid] = 0;
        __syncthreads();
        const uint32_t prefix = s_prefix, sh = 8u * (uint32_t)pass;
#pragma unroll
        for (int j = 0; j < KPT; ++j) {
            const uint32_t v = mine[j];
            if (j * 256 + tid < K && v <= T0 && (pass == 3 || (v >> (sh + 8u)) == prefix)) {
                // the lanes that share the first lane's digit add ONE count (the top digits of distances are all but equal)
                const uint32_t dg = (v >> sh) & 255u;
                const uint32_t lead = (uint32_t)__builtin_amdgcn_readfirstlane((int)dg);
                if (dg == lead) {
                    const uint64_t same = __builtin_amdgcn_ballot_w64(true);
                    if (__builtin_amdgcn_mbcnt_hi((uint32_t)(same >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)same, 0u)) == 0)
                        atomicAdd(&hist[lead], (uint32_t)__popcll(same));
                } else {
                    atomicAdd(&hist[dg], 1u);
                }
            }
        }
        __syncthreads();
        if (tid < 64) {                                          // wave 0: 4 bins per lane, the digit that holds rank s_rank
            const uint32_t c0 = hist[4 * tid], c1 = hist[4 * tid + 1], c2 = hist[4 * tid + 2], c3 = hist[4 * tid + 3];
            const uint32_t sum4 = c0 + c1 + c2 + c3;
            const uint32_t incl = dpp_wave_incl_sum(sum4), excl = incl - sum4;
            const uint32_t r = s_rank;
            if (incl >= r && excl < r) {                         // exactly one lane
                uint32_t run = excl, digit = 4 * tid;
                const uint32_t cs4[4] = {c0, c1, c2, c3};
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    if (run + cs4[jj] >= r) { digit = 4 * tid + jj; break; }
                    run += cs4[jj];
                }
                s_prefix = (prefix << 8) | digit;
                s_rank = r - run;                                // rank inside the chosen digit
            }
        }
        __syncthreads();
    }
    const uint32_t T = s_prefix, need_ties = s_rank;            // need_ties keys equal to T complete the ma smallest
#pragma unroll
    for (int j = 0; j < KPT; ++j) {
        const uint32_t v = mine[j], k = (uint32_t)(j * 256 + tid);
        if (k >= (uint32_t)K) continue;
        if (v < T) cand[atomicAdd(&s_nless, 1u)] = ((uint64_t)v << 32) | k;
        else if (v == T) {
            const uint32_t slot = atomicAdd(&s_nties, 1u);
            if (slot < 256u) ties[slot] = k;
        }
    }
    __syncthreads();
    const uint32_t nless = s_nless, nties = s_nties;            // nless == ma - need_ties
    __shared__ uint32_t s_tie;
    if (nties > need_ties) {                                     // a value equal to the ma-th outside the picks: an exact tie at the boundary —
        // the reference's heap history decides which of them stay and in which order (coarse_exact_select); uniform branch
        if (tid < 64) coarse_exact_select(dist + (size_t)q * K, K, ma, assign + (size_t)q * ma, x_hv, x_hk, x_perm, (uint32_t)tid);
        return;
    }
    if (tid == 0) s_tie = 0;
    // ties: the need_ties smallest indices among them; then the ma survivors in (distance, index) order.  Both by COUNTING — an
    // entry's place is the number of smaller entries, read as LDS broadcasts (indices and keys are distinct) — instead of two
    // 256-element bitonic networks: 72 barrier steps were most of this kernel (87 us alone on the GPU at the C5 shape for 67 MB of
    // distances; round 4).
    if ((uint32_t)tid < nties) {
        const uint32_t mine_k = ties[tid];
        uint32_t rank = 0;
        for (uint32_t j = 0; j < nties; ++j) rank += ties[j] < mine_k ? 1u : 0u;
        if (rank < need_ties) cand[nless + rank] = ((uint64_t)T << 32) | mine_k;
    }
    __syncthreads();
    if (tid < ma) {
        const uint64_t key = cand[tid];
        const uint32_t kv = (uint32_t)(key >> 32);
        uint32_t rank = 0, same = 0;
        int j = 0;
        for (; j + 2 <= ma; j += 2) {                            // (two keys per LDS read)
            const ulonglong2 kk = *reinterpret_cast<const ulonglong2*>(&cand[j]);
            rank += (kk.x < key ? 1u : 0u) + (kk.y < key ? 1u : 0u);
            same += ((uint32_t)(kk.x >> 32) == kv ? 1u : 0u) + ((uint32_t)(kk.y >> 32) == kv ? 1u : 0u);
        }
        for (; j < ma; ++j) {
            rank += cand[j] < key ? 1u : 0u;
            same += (uint32_t)(cand[j] >> 32) == kv ? 1u : 0u;
        }
        assign[(size_t)q * ma + rank] = (int32_t)(uint32_t)key;
        if (same > 1u) s_tie = 1u;                               // two picks with the same distance: an exact tie inside
    }
    __syncthreads();
    if (s_tie && tid < 64) coarse_exact_select(dist + (size_t)q * K, K, ma, assign + (size_t)q * ma, x_hv, x_hk, x_perm, (uint32_t)tid);
}

hipError_t coarse_nan_unreplayed_reset(hipStream_t stream) {
    const unsigned int zero = 0;
    return hipMemcpyToSymbolAsync(HIP_SYMBOL(g_coarse_nan_unreplayed), &zero, sizeof(zero), 0, hipMemcpyHostToDevice, stream);
}

hipError_t coarse_nan_unreplayed_read(unsigned int* count) {
    return hipMemcpyFromSymbol(count, HIP_SYMBOL(g_coarse_nan_unreplayed), sizeof(*count), 0, hipMemcpyDeviceToHost);
}

void launch_row_sqnorm(const float* d_rows, int n, int dim, int sum_mode, float* d_out, hipStream_t stream) {
    if (n > 0) hipLaunchKernelGGL(row_sqnorm_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, d_rows, n, dim, sum_mode, d_out);
}

void launch_coarse_assign(const float* d_queries, const float* d_coarse, int nq, int K, int dim, int ma, float* d_qnorm,
                          const float* d_cnorm, int sum_mode, float* d_dist, int32_t* d_assign, hipStream_t stream) {
    const int kpt = (K + 255) / 256;
    launch_row_sqnorm(d_queries, nq, dim, sum_mode, d_qnorm, stream);                       // ||q||^2 (the centroids': the caller's, once)
    // large batches share every centroid row between 4 queries (registers: KPT x 4 distances per thread)
#define QADC_CA(N, QB) hipLaunchKernelGGL((coarse_assign_kernel<N, QB>), dim3((nq + QB - 1) / QB), dim3(256), (size_t)QB * dim * sizeof(float), \
                                          stream, d_queries, d_coarse, nq, K, dim, ma, d_qnorm, d_cnorm, d_dist, d_assign)
    // (any batch size: even one query — 15 of its group's 16 rows idle — is through sooner than with a row per lane)
    if (kpt <= 64 && ma <= K && dim % 4 == 0 && (reinterpret_cast<uintptr_t>(d_coarse) & 15) == 0 && d_dist) {
        hipLaunchKernelGGL(coarse_dist_kernel, dim3(kpt, (nq + kCDQ - 1) / kCDQ), dim3(256), 0, stream, d_queries, d_coarse, nq, K, dim, d_qnorm,
                           d_cnorm, d_dist);
        if (ma <= 256 && ma >= 8) {                              // radix select + one sort (few probes: the rounds are as quick)
            if (kpt <= 4) hipLaunchKernelGGL(coarse_select_radix_kernel<4>, dim3(nq), dim3(256), 0, stream, d_dist, K, ma, d_assign);
            else if (kpt <= 16) hipLaunchKernelGGL(coarse_select_radix_kernel<16>, dim3(nq), dim3(256), 0, stream, d_dist, K, ma, d_assign);
            else hipLaunchKernelGGL(coarse_select_radix_kernel<64>, dim3(nq), dim3(256), 0, stream, d_dist, K, ma, d_assign);
        }
        else if (kpt <= 4) hipLaunchKernelGGL(coarse_select_kernel<4>, dim3(nq), dim3(256), 0, stream, d_dist, K, ma, d_assign);
        else if (kpt <= 16) hipLaunchKernelGGL(coarse_select_kernel<16>, dim3(nq), dim3(256), 0, stream, d_dist, K, ma, d_assign);
        else hipLaunchKernelGGL(coarse_select_kernel<64>, dim3(nq), dim3(256), 0, stream, d_dist, K, ma, d_assign);
    } else if (nq >= 512) {
        if (kpt <= 4) QADC_CA(4, 4);
        else if (kpt <= 16) QADC_CA(16, 4);
        else if (kpt <= 32) QADC_CA(32, 2);
        else QADC_CA(0, 4);
    } else {
        if (kpt <= 4) QADC_CA(4, 1);
        else if (kpt <= 16) QADC_CA(16, 1);
        else if (kpt <= 32) QADC_CA(32, 1);
        else QADC_CA(0, 1);
    }
#undef QADC_CA
}

__global__ __launch_bounds__(256) void build_tables_kernel(const float* __restrict__ queries, const float* __restrict__ coarse,
                                                           const int32_t* __restrict__ assign,
                                                           const float* __restrict__ codebooks,
                                                           const float* __restrict__ rotation, int ma, int M, int dim,
                                                           int expansion, int sum_mode, float* __restrict__ ftables) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
    float* res = reinterpret_cast<float*>(dyn);               // [dim] residual of this (query, probe)
    float* tmp = res + dim;                                   // [dim] un-rotated residual (OPQ only)
    const int a = blockIdx.x, qi = blockIdx.y, tid = threadIdx.x;
    const int ds = dim / M;
    const float* __restrict__ c = coarse ? coarse + (size_t)assign[(size_t)qi * ma + a] * dim : nullptr;
    float* first = rotation ? tmp : res;
    for (int d = tid; d < dim; d += 256) {
        const float x = queries[(size_t)qi * dim + d];
        first[d] = c ? x - c[d] : x;
    }
    __syncthreads();
    if (rotation) {
        // opq::rotate_multiple_vectors (quantizers.hpp:289-301): rotated[r] = sum_c x[c] * rotation[r][c]
        for (int r = tid; r < dim; r += 256) {
            const float* __restrict__ row = rotation + (size_t)r * dim;
            float acc = 0.0f;
            for (int cc = 0; cc < dim; ++cc) acc += tmp[cc] * row[cc];
            res[r] = acc;
        }
        __syncthreads();
    }
    float* __restrict__ out = ftables + ((size_t)qi * ma + a) * (M * 16);
    for (int e = tid; e < M * 16; e += 256) {
        const int m = e >> 4;
        const float* __restrict__ ce = codebooks + (size_t)e * ds;   // [m][c][ds] is contiguous in e
        float s = 0.0f;
        if (expansion) {
            // compute_cross_dists_blas (distances.hpp:151-183): ||v||^2 + ||c||^2, then sgemm(alpha = -2, beta = 1) adds
            // -2 v.c: the BLAS-expansion form nns_engine uses for ma > 1 and nns_engine_batch always.  It can come out
            // slightly NEGATIVE when v ~ c — the case query_scan clamps (db_query_4.cpp:258-269).  Norms as compiled,
            // sequential dot, no contraction (expansion_dist above); host twin: pq4::tables_blas.
            const float* __restrict__ v = res + m * ds;
            s = expansion_dist(v, ce, ds, expansion_sqnorm(v, ds, sum_mode), expansion_sqnorm(ce, ds, sum_mode));
        } else {
            s = direct_sqdist(res + m * ds, ce, ds, sum_mode);
        }
        out[e] = s;
    }
}

// The same tables for kBTProbes (16; 8 and 32 within 15 %) probes of a query per workgroup (no OPQ rotation, sub-vectors of <= 8 components): a thread
// keeps its table entry's codebook row in registers and walks the probes, whose residuals wait in LDS.  One workgroup per
// (query, probe) is 65 K workgroups of 512 results each at the C5 shape — the launch was bound by workgroup dispatch and by
// re-reading the codebook row per result (92 us alone on the GPU for 134 MB of tables; round 4: -> 8 K workgroups).
// Entry for entry the arithmetic of build_tables_kernel: the same residual, the same sums in the same grouping.
constexpr int kBTProbes = 16;
__global__ __launch_bounds__(256) void build_tables_multi_kernel(const float* __restrict__ queries, const float* __restrict__ coarse,
                                                                 const int32_t* __restrict__ assign,
                                                                 const float* __restrict__ codebooks, int ma, int M, int dim,
                                                                 int expansion, int sum_mode, float* __restrict__ ftables) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
    float* res = reinterpret_cast<float*>(dyn);               // [kBTProbes][dim] residuals of this query's probes a0 ..
    const int a0 = blockIdx.x * kBTProbes, qi = blockIdx.y, tid = threadIdx.x;
    const int na = min(kBTProbes, ma - a0);
    const int ds = dim / M;
    for (int i = tid; i < na * dim; i += 256) {
        const int a = i / dim, d = i - a * dim;
        const float x = queries[(size_t)qi * dim + d];
        res[i] = coarse ? x - coarse[(size_t)assign[(size_t)qi * ma + a0 + a] * dim + d] : x;
    }
    __syncthreads();
    for (int e = tid; e < M * 16; e += 256) {
        const int m = e >> 4;
        float ce[8];
#pragma unroll
        for (int d = 0; d < 8; ++d) ce[d] = d < ds ? codebooks[(size_t)e * ds + d] : 0.0f;
        // (expansion form: ||c||^2 does not depend on the probe; constant ds so that the lane loops unroll over the registers)
        const float cn = !expansion ? 0.0f : ds == 8 ? expansion_sqnorm(ce, 8, sum_mode) : ds == 4 ? expansion_sqnorm(ce, 4, sum_mode)
                                                                                          : expansion_sqnorm(ce, ds, 0);
        for (int a = 0; a < na; ++a) {
            const float* __restrict__ r = res + a * dim + m * ds;
            float s = 0.0f;
            if (expansion) {
                const float vn = ds == 8 ? expansion_sqnorm(r, 8, sum_mode) : ds == 4 ? expansion_sqnorm(r, 4, sum_mode) : expansion_sqnorm(r, ds, 0);
                float dot = 0.0f;
#pragma unroll
                for (int d = 0; d < 8; ++d)
                    if (d < ds) dot += r[d] * ce[d];
                s = (vn + cn) + (-2.0f * dot);
            } else if (ds == 8) {
                s = direct_sqdist(r, ce, 8, sum_mode);               // (constant ds: the block loop unrolls over the registers)
            } else if (ds == 4) {
                s = direct_sqdist(r, ce, 4, sum_mode);
            } else {
#pragma unroll
                for (int d = 0; d < 8; ++d)                          // other ds <= 8: no instance in the reference — sequential
                    if (d < ds) {
                        const float t_ = r[d] - ce[d];
                        s += t_ * t_;
                    }
            }
            ftables[((size_t)qi * ma + a0 + a) * (M * 16) + e] = s;
        }
    }
}

void launch_build_tables(const float* d_queries, const float* d_coarse, const int32_t* d_assign, const float* d_codebooks,
                         const float* d_rotation, int nq, int ma, int M, int dim, int expansion, int sum_mode, float* d_ftables,
                         hipStream_t stream) {
    if (!d_rotation && dim / M <= 8 && ma > 1) {
        hipLaunchKernelGGL(build_tables_multi_kernel, dim3((ma + kBTProbes - 1) / kBTProbes, nq), dim3(256),
                           (size_t)kBTProbes * dim * sizeof(float), stream, d_queries, d_coarse, d_assign, d_codebooks, ma, M, dim,
                           expansion, sum_mode, d_ftables);
        return;
    }
    hipLaunchKernelGGL(build_tables_kernel, dim3(ma, nq), dim3(256), 2 * dim * sizeof(float), stream, d_queries, d_coarse,
                       d_assign, d_codebooks, d_rotation, ma, M, dim, expansion, sum_mode, d_ftables);
}

// ---------------------------------------------------------------------------------------------
// PQ encoder (base_pq::encode_multiple_vectors, quantizers.hpp:222-245): per sub-quantizer
// find_k_neighbors(count, 16, sq_dim, k = 1, ...) (neighbors.cpp:30-76) — the BLAS-expansion distances of
// compute_cross_dists_blas (expansion_dist above) pushed in centroid order into a kv_binheap of capacity 1
// (add_candidates_heaps, 18-28; binheap.hpp:75-116): the first centroid is appended whatever its distance, a later one
// replaces it iff !(distance >= kept) — the replace test AS COMPILED (-ffast-math: vcomiss + jae; oracle/qadc_oracle.c
// orc_select_k_neighbors): the first strict minimum after the last NaN, or the last centroid when its distance is NaN.
// LDS: the codebooks (+ their norms for form 1), up to dim 2048 = 128 KiB + 2 KiB: above 64 KiB the launch raises the kernel's
// dynamic-LDS limit (hipFuncAttributeMaxDynamicSharedMemorySize; gfx950 has 160 KiB per workgroup).
// Two sub-quantizers per byte, the even one in the low nibble (multiple_set_bits_4, quantizers.hpp:49-68).
// form 1 = that (the reference's form; parity: the oracle's orc_pq_encode, tests/test_gpu_parity.py); form 0 = the direct
// sum (x - c)^2 in one sequential loop (this repository's encoder before round 6).  One thread per code byte.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pq_encode_kernel(const float* __restrict__ vectors, uint64_t n, int M, int dim,
                                                        const float* __restrict__ codebooks, int form, int sum_mode,
                                                        uint8_t* __restrict__ codes) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
    float* cb = reinterpret_cast<float*>(dyn);                // [M][16][ds]
    float* cnorm = cb + (size_t)M * 16 * (dim / M);           // [M][16] ||c||^2 (form 1 only: not allocated for form 0)
    const int ds = dim / M, cs = M / 2;
    for (int i = threadIdx.x; i < M * 16 * ds; i += 256) cb[i] = codebooks[i];
    __syncthreads();
    if (form) {
        for (int e = threadIdx.x; e < M * 16; e += 256) cnorm[e] = expansion_sqnorm(cb + (size_t)e * ds, ds, sum_mode);
        __syncthreads();
    }
    const uint64_t total = n * (uint64_t)cs;
    for (uint64_t o = (uint64_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (uint64_t)gridDim.x * 256) {
        const uint64_t vi = o / cs;
        const int b = (int)(o % cs);
        uint32_t packed = 0;
        for (int h = 0; h < 2; ++h) {
            const int m = 2 * b + h;
            const float* __restrict__ x = vectors + vi * dim + (uint64_t)m * ds;
            const float vn = form ? expansion_sqnorm(x, ds, sum_mode) : 0.0f;
            int best = 0;
            float bestd = 0.0f;
            for (int c = 0; c < 16; ++c) {
                const float* ce = cb + ((size_t)m * 16 + c) * ds;
                float s = 0.0f;
                if (form) {
                    s = expansion_dist(x, ce, ds, vn, cnorm[m * 16 + c]);
                } else {
                    for (int d = 0; d < ds; ++d) {
                        const float t = x[d] - ce[d];
                        s += t * t;
                    }
                }
                if (c == 0 || !(s >= bestd)) { bestd = s; best = c; }   // (the compiled replace test, see above)
            }
            packed |= (uint32_t)best << (4 * h);
        }
        codes[o] = (uint8_t)packed;
    }
}

void launch_pq_encode(const float* d_vectors, uint64_t n, int M, int dim, const float* d_codebooks, int form, int sum_mode,
                      uint8_t* d_codes, hipStream_t stream) {
    const uint64_t total = n * (uint64_t)(M / 2);
    const int grid = (int)std::min<uint64_t>((total + 255) / 256, 16384);
    const size_t lds = ((size_t)M * 16 * (dim / M) + (form ? (size_t)M * 16 : 0)) * sizeof(float);
    static std::atomic<uint64_t> lds_set{0};
    if (lds > 65536) ensure_dynamic_lds(reinterpret_cast<const void*>(&pq_encode_kernel), (int)kPqEncodeMaxLds, lds_set);
    hipLaunchKernelGGL(pq_encode_kernel, dim3(grid), dim3(256), lds, stream, d_vectors, n, M, dim, d_codebooks, form, sum_mode, d_codes);
}

// ---------------------------------------------------------------------------------------------
// Database build.  index_db::add_vectors (databases.hpp:270-298): nearest coarse centroid
// (coarse_dist_kernel + coarse_select_kernel with ma = 1), then per vector the residual x - centroid and, for OPQ, the
// rotation rotated[r] = sum_c x[c] * rotation[r][c] (quantizers.hpp:289-301) in sequential float sums — the same loops as
// build_tables_kernel and host/query_driver.hpp — and pq_encode_kernel on the result.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void residual_rotate_kernel(const float* __restrict__ vectors, uint64_t n, int dim,
                                                              const float* __restrict__ coarse, const int32_t* __restrict__ assign,
                                                              const float* __restrict__ rotation, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
    float* res = reinterpret_cast<float*>(dyn);                  // [dim] residual of this workgroup's vector
    for (uint64_t v = blockIdx.x; v < n; v += gridDim.x) {
        const float* __restrict__ x = vectors + v * dim;
        const float* __restrict__ c = coarse ? coarse + (size_t)assign[v] * dim : nullptr;
        __syncthreads();
        for (int d = threadIdx.x; d < dim; d += 256) res[d] = c ? x[d] - c[d] : x[d];
        __syncthreads();
        for (int r = threadIdx.x; r < dim; r += 256) {
            float o = res[r];
            if (rotation) {
                const float* __restrict__ row = rotation + (size_t)r * dim;
                o = 0.0f;
                for (int cc = 0; cc < dim; ++cc) o += res[cc] * row[cc];
            }
            out[v * dim + r] = o;
        }
    }
}

void launch_residual_rotate(const float* d_vectors, uint64_t n, int dim, const float* d_coarse, const int32_t* d_assign,
                            const float* d_rotation, float* d_out, hipStream_t stream) {
    if (!n) return;
    hipLaunchKernelGGL(residual_rotate_kernel, dim3((unsigned)std::min<uint64_t>(n, 65536)), dim3(256), (size_t)dim * sizeof(float),
                       stream, d_vectors, n, dim, d_coarse, d_assign, d_rotation, d_out);
}

// kmeans_fast_iterations_thread's centroid update (databases.cpp:67-88): centroid = (sum of its members, added in
// ascending vector order) / member count; an empty cluster divides 0 by 0 like the reference does.  One workgroup per
// centroid walks assign[] in order, compacts the members of every 256-vector chunk IN ORDER (ballot + prefix) and
// lets its lanes (one per component) add them sequentially: the float sums are those of the sequential host loop.
// div_mode 1 (default) — AS COMPILED: the reference is built with -ffast-math, and g++ turns the loop's division by the member
// count (databases.cpp:83-88) into one reciprocal 1.0f / (float)count and a multiplication per component (pinned to the
// reference's own loops compiled here: oracle/_ref, qadc_reff_kmeans_update); 0 — the source's division.
__global__ __launch_bounds__(256) void kmeans_update_kernel(const float* __restrict__ vectors, uint64_t n, int dim,
                                                            const int32_t* __restrict__ assign, float* __restrict__ centroids,
                                                            int div_mode) {
    __shared__ uint32_t members[256];
    __shared__ uint32_t wcount[4];
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int kMaxPer = 8;                                   // components per lane (dim <= 2048)
    float acc[kMaxPer];
#pragma unroll
    for (int j = 0; j < kMaxPer; ++j) acc[j] = 0.0f;
    uint32_t count = 0;
    for (uint64_t base = 0; base < n; base += 256) {
        const uint64_t i = base + tid;
        const bool mine = i < n && assign[i] == c;
        const uint64_t m = __builtin_amdgcn_ballot_w64(mine);
        if (lane == 0) wcount[wave] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t before = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u)), total = 0;
        for (int w = 0; w < 4; ++w) {
            if (w < wave) before += wcount[w];
            total += wcount[w];
        }
        if (mine) members[before] = (uint32_t)(i - base);
        __syncthreads();
        for (uint32_t k = 0; k < total; ++k) {
            const float* __restrict__ x = vectors + (base + members[k]) * dim;
#pragma unroll
            for (int j = 0; j < kMaxPer; ++j) {
                const int d = tid + 256 * j;
                if (d < dim) acc[j] += x[d];
            }
        }
        count += total;
    }
#pragma unroll
    for (int j = 0; j < kMaxPer; ++j) {
        const int d = tid + 256 * j;
        if (d < dim) centroids[(size_t)c * dim + d] = div_mode ? acc[j] * (1.0f / (float)(int)count) : acc[j] / (float)(int)count;
    }
}

void launch_kmeans_update(const float* d_vectors, uint64_t n, int dim, int K, const int32_t* d_assign, float* d_centroids,
                          int div_mode, hipStream_t stream) {
    hipLaunchKernelGGL(kmeans_update_kernel, dim3(K), dim3(256), 0, stream, d_vectors, n, dim, d_assign, d_centroids, div_mode);
}

// ---------------------------------------------------------------------------------------------
// Synthetic codes: word w (8 code bytes) = splitmix64(seed ^ splitmix64(w)), little endian.
// Same function as orc_fill_codes in the oracle, so any sub-range is reproducible on the CPU.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

__global__ __launch_bounds__(256) void fill_codes_kernel(uint64_t* __restrict__ dst, uint64_t first_word, uint64_t nwords,
                                                         uint64_t seed) {
    for (uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x; w < nwords; w += (uint64_t)gridDim.x * 256)
        dst[w] = splitmix64(seed ^ splitmix64(first_word + w));
}

void launch_fill_codes(uint8_t* d_dst, uint64_t first_word, uint64_t nwords, uint64_t seed, hipStream_t stream) {
    const int grid = (int)std::min<uint64_t>((nwords + 255) / 256, 8192);
    hipLaunchKernelGGL(fill_codes_kernel, dim3(grid), dim3(256), 0, stream, reinterpret_cast<uint64_t*>(d_dst), first_word,
                       nwords, seed);
}

// Reference block layout [B][cs][16] (simd_layout.hpp:41-65) -> device row-major [n][cs].
__global__ __launch_bounds__(256) void deinterleave_kernel(uint8_t* __restrict__ rowmajor, const uint8_t* __restrict__ inter,
                                                           uint32_t n, int cs) {
    const uint64_t total = (uint64_t)n * cs;
    for (uint64_t o = (uint64_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (uint64_t)gridDim.x * 256) {
        const uint64_t ci = o / cs;
        const int b = (int)(o % cs);
        rowmajor[o] = inter[(ci / 16) * cs * 16 + (uint64_t)b * 16 + (ci % 16)];
    }
}

void launch_deinterleave(uint8_t* d_rowmajor, const uint8_t* d_inter, uint32_t n, int cs, hipStream_t stream) {
    const uint64_t total = (uint64_t)n * cs;
    const int grid = (int)std::min<uint64_t>((total + 255) / 256, 8192);
    hipLaunchKernelGGL(deinterleave_kernel, dim3(grid), dim3(256), 0, stream, d_rowmajor, d_inter, n, cs);
}

}  // namespace qadc
