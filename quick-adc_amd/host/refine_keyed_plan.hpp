// The keyed refine store's table (qadc_refine_create_keyed, _put, _remove): the hash, the sizing rule, the
// rebuild rule, the pass sizes and the launch geometry — HIP-free, so that tests/cpp/refine_keyed_plan_host.cpp can sweep it on the
// CPU.  csrc/qadc_refine.cpp plans every put, remove and reserve with these functions and the kernels of csrc/qadc_refine_kernel.hip
// use keyed_slot.
//
// The table has 2^bits slots (key, row) with linear probing from keyed_slot(key, bits).  A slot is EMPTY (key 0xFFFFFFFF), LIVE
// (a key and its row) or DEAD (a removed key, kept so that probe chains stay whole, row = none).  used = live + dead slots.
//
// Invariant: used <= slots / 2 at all times, so every probe meets an empty slot.
//
// A put of `count` inputs first counts, with one kernel over the whole call, the inputs whose key the table does not know
// (neither live nor dead): `absent`, an upper bound of the slots the call can claim — a key listed twice is counted twice.  Then
// plan_put decides, before the first pass, whether the table is rebuilt; no pass rebuilds.  A call that only overwrites has
// absent = 0 and never rebuilds.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define QADC_KEYED_HD __host__ __device__
#else
#define QADC_KEYED_HD
#endif

namespace qadc {
namespace refine {

constexpr uint32_t kKeyedEmpty = 0xFFFFFFFFu;        // the key of an empty slot and of a free row; never a caller's key
constexpr uint32_t kKeyedNoRow = 0xFFFFFFFFu;        // the row field of an empty or dead slot
constexpr int kKeyedMinBits = 10;                    // the smallest table: 1024 slots
constexpr int kKeyedMaxBits = 31;                    // the largest: 2^31 slots, so at most 2^30 keys live and dead
constexpr uint64_t kKeyedMaxKeys = 1ull << 30;       // live keys a store takes (and rows it allocates)
constexpr uint64_t kKeyedPass = 1ull << 20;          // inputs of one pass of a put or a remove: bounds the call's device scratch
constexpr uint64_t kKeyedPassFloats = 1ull << 24;    // ... and the floats of host memory a pass of a put uploads (64 MiB)
constexpr int kKeyedThreads = 256;                   // threads of a workgroup of every keyed kernel, one input (or row, or slot) each
constexpr unsigned kKeyedMaxGrid = 65536;            // workgroups of a launch at most (the kernels stride over what is left)
constexpr size_t kKeyedSlotBytes = 12;               // key, row and the put's scratch word of a slot

// The home slot of a key in a table of 2^bits slots: the upper `bits` bits of the 32-bit finalizer of MurmurHash3.  bits <= 0
// gives 0 and bits >= 32 the whole hash.
QADC_KEYED_HD inline uint32_t keyed_slot(uint32_t key, int bits) {
    uint32_t h = key;
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return bits <= 0 ? 0u : bits >= 32 ? h : h >> (32 - bits);
}

// The smallest table that holds `keys` used slots in half of it: the least bits >= kKeyedMinBits with 2^bits >= 2 * keys; 0 where
// none does (keys above 2^30).
inline int keyed_bits_for(uint64_t keys) {
    for (int bits = kKeyedMinBits; bits <= kKeyedMaxBits; ++bits)
        if ((1ull << bits) >= 2 * keys) return bits;
    return 0;
}

struct KeyedPutPlan {
    bool refused;       // the call would pass kKeyedMaxKeys
    bool rebuild;       // the table is rebuilt (or first built) before the first pass
    int bits;           // the table's size during and after the call
};

// The table before a put: `bits` (0 = no table yet) with `live` and `dead` slots used; `absent` as counted for the call.  The
// call's claims fit where used + absent <= slots / 2.  Otherwise the table is rebuilt from the live rows, which drops the dead
// slots, for live + absent keys and a quarter of the live ones more, so that a store whose puts and removes keep it near one size
// is not rebuilt by every call.
inline KeyedPutPlan plan_put(int bits, uint64_t live, uint64_t dead, uint64_t absent) {
    KeyedPutPlan p{false, false, bits};
    if (live + absent > kKeyedMaxKeys) {
        p.refused = true;
        return p;
    }
    if (bits && live + dead + absent <= (1ull << bits) / 2) return p;
    p.rebuild = true;
    p.bits = std::max(bits, keyed_bits_for(std::min<uint64_t>(live + absent + live / 4, kKeyedMaxKeys)));   // (a table never shrinks)
    return p;
}

// qadc_refine_reserve(rows) on a keyed store: the table that takes `rows` live keys, never a smaller one than there is; a rebuild
// where it grows.  Puts that keep live + dead + absent <= rows afterwards plan no rebuild.
inline KeyedPutPlan plan_reserve(int bits, uint64_t rows) {
    KeyedPutPlan p{rows > kKeyedMaxKeys, false, bits};
    if (p.refused) return p;
    const int want = keyed_bits_for(rows);
    if (want > bits) {
        p.rebuild = true;
        p.bits = want;
    }
    return p;
}

// The passes of a call of `count` inputs of `dim` floats each (dim 0: a remove, which uploads keys only): pass i takes the inputs
// [i * keyed_pass(dim), min(count, (i + 1) * keyed_pass(dim))).
inline uint64_t keyed_pass(int dim) {
    if (dim <= 0) return kKeyedPass;
    return std::max<uint64_t>(1, std::min<uint64_t>(kKeyedPass, kKeyedPassFloats / (uint64_t)dim));
}

// workgroups of kKeyedThreads threads for n items (inputs, rows, slots or row components), at least 1
inline unsigned keyed_grid(uint64_t n) {
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + kKeyedThreads - 1) / kKeyedThreads, kKeyedMaxGrid));
}

}  // namespace refine
}  // namespace qadc
