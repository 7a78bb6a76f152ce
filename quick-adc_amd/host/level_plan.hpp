// The planner of the int8 level path: integer arithmetic on the partition table, the options and
// the probe lists of a batch.  Every exactness argument of that section rests on what it emits — the level cuts, the 16-byte
// alignment of every run, the 2^31 cut, dup_pos / dup_reps, which runs may take the split form, the pre-scan items — and it also
// picks kernel and grid of every level launch.  No HIP here, and no pointer is dereferenced (the device pointers are only offset):
// csrc/qadc_kernels.h and csrc/qadc_host.h include this header for the item and launch structs, csrc/qadc_capi.cpp plans every
// level-path batch with plan_levels, and tests/cpp/level_plan_host.cpp checks the plan's invariants on a CPU.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace qadc {

// One contiguous run of codes of one probed partition, scanned with one int8 table.
// (A probed partition is cut into one item per bound level, see DESIGN.md "Exact filtering".)
struct ScanItem {
    const uint8_t* codes;    // first code of the run (16-byte aligned)
    const uint32_t* labels;  // partition labels (indexed by position in partition) or nullptr
    uint32_t n;              // codes in the run
    uint32_t pos0;           // position of the first code inside its partition
    uint32_t key_base;       // added to the position when labels == nullptr (shard offset)
    uint32_t table;          // table index: qtables + table * M * 16
    uint32_t query;          // per-query state index
    uint32_t order;          // (level << 16) | assign slot (< 2^14): scan-order major key of emitted entries
    uint32_t dup_pos;        // position (in the partition) of the code the reference replays in its padding
                             // lanes, if this run's partition end is held here; else 0xffffffff
    uint32_t dup_reps;       // number of extra replays of that code: (16 - n % 16) % 16
    const uint8_t* split;    // 16x4: the run's first tile in the partition's byte-plane copy (launch_split_copy), or nullptr; in a
                             // launch of the nibble form (LevelLaunch::nib): that tile in the nibble-plane copy (launch_nib_copy)
                             // In a launch of the bucket form (LevelLaunch::bkt): the run's first tile in the bucket copy's planes; codes =
                             // that tile in the copy's per-slot side array (kBktSideBytes per tile), n = the run's SLOTS (whole tiles)
};

// Byte-plane copy of code bytes 0-6 (16x4 only), the input of the split form of scan_i8_kernel: tile t of a partition holds
// codes [t * kSplitTile, (t + 1) * kSplitTile) as 7 planes of kSplitTile bytes each (plane b = byte b of consecutive codes) at
// byte t * 7 * kSplitTile.  One tile is one workgroup iteration of the split form: 1024 lanes x 16 codes.  Padded to whole
// tiles (codes past the partition's end read as 0).  Byte 7 stays in the row-major array only.
constexpr uint32_t kSplitTile = 16384;
constexpr uint32_t kSplitBytes = 7;
// Nibble-plane copy (16x4 only), the input of scan_i8_nib_kernel: the same kSplitTile-code tiles, 16 planes of kSplitTile / 2
// bytes each at byte t * kNibTileBytes; plane s = sub-quantizer s of the tile's codes at half a byte each (8 bytes per code: byte 7
// has its planes too).  A lane's 16 codes are the two dwords at byte 8 * lane of a plane; in a dword, codes 0-3 of its eight are the
// low nibbles of bytes 0-3 and codes 4-7 the high nibbles, so two planes merge into eight pair-table indices with two
// bit-field inserts.  Padded to whole tiles with zeros.
constexpr uint32_t kNibTileBytes = 8 * kSplitTile;
// The nibble form's choice bytes of one table: 4 bytes for each NS = 8, 9, 10 streamed sub-quantizers at 4 * (NS - 8):
// the deferred set as a 16-bit mask (low byte first), the slack c, 0.
constexpr uint32_t kNibSelBytes = 12;

// Bucket copy (16x4 only), the input of scan_i8_bkt_kernel.  A partition is cut into blocks of bkt_block codes from its first code
// (the last may be short); inside a block the codes are grouped by key = code byte 0 | code byte 1 << 8 (sub-quantizers 0-3).
// Every non-empty bucket is padded to a multiple of 16 slots with copies of its last code, and the block to whole kSplitTile-slot
// tiles with copies of its last code, so every 16-slot lane group has ONE key.  Tile t of the copy holds slots
// [t * kSplitTile, (t + 1) * kSplitTile): 12 nibble planes of kSplitTile / 2 bytes (sub-quantizers 4-15, the nibble copy's
// in-plane layout), then the id plane, one uint16 key per 16-slot group.  Beside it, per tile, the side array: the slots' 8-byte
// codes (read by survivors), then their uint32 positions in the partition (perm; read by candidates; a padding slot: kBktPad).
constexpr uint32_t kBktPlanes = 12;
constexpr uint32_t kBktIdOff = kBktPlanes * (kSplitTile / 2);                  // byte offset of the id plane in a tile
constexpr uint32_t kBktTileBytes = kBktIdOff + kSplitTile / 16 * 2;
constexpr uint32_t kBktPermOff = 8 * kSplitTile;                               // byte offset of perm in a tile of the side array
constexpr uint32_t kBktSideBytes = kBktPermOff + 4 * kSplitTile;
constexpr uint32_t kBktPad = 0xffffffffu;
constexpr uint32_t kBktKeys = 65536;
// The bucket form's choice bytes of one table: 4 bytes for each NSP = 4, 5, 6, 7 paid sub-quantizers at 4 * (NSP - 4): the
// deferred set among sub-quantizers 4-15 as a 16-bit mask (low byte first), the slack c, 0.
constexpr uint32_t kBktSelBytes = 16;
// Wide blocks of the bucket copy.  From position bkt_wide_block = W on, a partition is cut into octave blocks [W 2^j, W 2^(j+1)),
// j = 0, 1, ... (the last clipped at the partition's end), and an octave is grouped by the 20-bit key = code bytes 0 and 1 and the
// low nibble of byte 2 (sub-quantizers 0-4); padding as in a narrow block.  Wide tiles live in an allocation of their own: 11 nibble
// planes (sub-quantizers 5-15, the same in-plane layout), then the id plane of the narrow tile (uint16 = sub-quantizers 0-3 of the
// 16-slot group), then one byte per group, sub-quantizer 4 of the group.  The side array has the narrow copy's layout.  A range
// that wide octaves cover has no slots in the narrow copy (its narrow blocks are empty); an octave whose padded slots exceed
// bkt_wide_max_pad x its codes has no slots in the wide copy, and narrow blocks instead.
constexpr uint32_t kBktwPlanes = 11;
constexpr uint32_t kBktwIdOff = kBktwPlanes * (kSplitTile / 2);                // byte offset of the uint16 id plane in a wide tile
constexpr uint32_t kBktwId4Off = kBktwIdOff + kSplitTile / 16 * 2;             // ... and of the byte plane of sub-quantizer 4
constexpr uint32_t kBktwTileBytes = kBktwId4Off + kSplitTile / 16;
constexpr uint32_t kBktwKeys = 1u << 20;
// The wide form's choice bytes of one table: 4 bytes for each NSP = 3, 4, 5, 6 paid sub-quantizers at 4 * (NSP - 3): the deferred
// set among sub-quantizers 5-15 as a 16-bit mask (low byte first), the slack c, 0.
constexpr uint32_t kBktwSelBytes = 16;

constexpr int kMaxLevels = 16;  // bound levels per query

// Float ADC item for the "starts" pre-scan (scanner_4::query_scan_start).
struct StartItem {
    const uint8_t* codes;  // first code of the partition
    uint32_t n;            // starts size of that partition
    uint32_t table;        // float table index: ftables + table * M * 16
    uint32_t query;
    uint32_t out_off;      // filter == 0: offset inside the query's float value buffer
    uint32_t filter;       // 1: append only values <= QueryState::qmax (the sample's R-th smallest)
};

namespace host {

// Fixed tuning constants (each was an option while it was being measured; the sweeps are in profiles/, see profiles/README.md)
constexpr uint32_t kShareCodesPerWg = 1u << 20;    // codes per workgroup of a sibling-major shared launch
constexpr uint32_t kMqCodesPerWg = 1u << 16;       // ... of a multi-query launch (8 queries per pass)
constexpr uint32_t kMqMinWgs = 4096;               // workgroups a multi-query launch should have at least (2 rounds of the chip)
constexpr uint32_t kMqMinTiles = 4;                // ... but never fewer than this many 4 KiB tiles per workgroup
constexpr uint32_t kSmallVecPerWg = 512;           // 16-byte vectors one small-run workgroup covers

struct LevelLaunch {
    size_t first;   // first item
    int nitems;
    int wgs;
    uint64_t codes;
    bool small;     // small-run kernel (runs below small_run codes)
    bool shared;    // every run of the launch covers the same codes (one run per query): sibling-major launch
    bool mq;        // ... and groups of 8 of them share one pass (scan_i8_mq_kernel)
    bool split;     // every run of the launch reads the byte-plane copy (split form of scan_i8_kernel)
    bool split6;    // ... and has at least split6_min_run codes: the 6-plane form (the query's table defers a second byte)
    uint64_t maxn;  // longest run of the launch
    bool early;     // launched on the front stream, under the previous batch's long levels: counted, not event-timed
    int ev = -1;    // index of the HIP event recorded before the launch (the next one follows it), -1 = not timed
    bool split5 = false;   // split, and every run has at least split5_min_run codes: the 5-plane form (the launcher prefers 5 over 6 over 7)
    int nib = 0;           // 8, 9 or 10: split, every run starts on a tile of its partition's nibble-plane copy and has at least the form's
                           // threshold of codes: scan_i8_nib_kernel streams that many of the 16 sub-quantizers (preferred over 5 planes); 0: not
    uint64_t slots = 0;    // bkt: the slots of the launch's runs (what it streams; codes stays what the runs cover)
    int bkt = 0;           // 4, 5, 6 or 7: split, every run covers whole blocks of its partition's bucket copy (bkt_run_ok): scan_i8_bkt_kernel
                           // streams that many of sub-quantizers 4-15 (preferred over the nibble form; nib is 0 then); 0: not.  The runs
                           // then count slots (ScanItem::n) and wgs derives from them; codes and maxn stay the codes the runs cover
    int bktw = 0;          // 3, 4, 5 or 6: split, every run covers whole wide octaves of its partition's bucket copy (bktw_run_ok): the wide
                           // form of scan_i8_bkt_kernel streams that many of sub-quantizers 5-15 (preferred over the narrow form; bkt and
                           // nib are 0 then); the runs count slots as in a narrow bucket launch
};

// What the planner reads of a partition (the index's Part derives from it: one partition table, no copy).
struct LevelPart {
    uint8_t* d_codes = nullptr;    // row-major codes of the local range
    uint32_t* d_labels = nullptr;  // labels of the local range (or null)
    uint8_t* d_starts = nullptr;   // replica of the global partition's first codes (null: d_codes, first_pos == 0)
    uint8_t* d_split = nullptr;    // 16x4: byte-plane copy of code bytes 0-6 for the split scan (kSplitTile), or null
    uint8_t* d_nib = nullptr;      // 16x4: nibble-plane copy of all 16 sub-quantizers (kNibTileBytes per tile), or null
    uint8_t* d_bkt = nullptr;      // 16x4: the bucket copy's tiles (kBktTileBytes per tile), or null
    uint8_t* d_bkt_side = nullptr; // ... and its side array (kBktSideBytes per tile)
    uint64_t bkt_block = 0;        // codes per block of the copy (a power of two, a multiple of kSplitTile)
    std::vector<uint64_t> bkt_off; // [blocks + 1] first slot of every block (multiples of kSplitTile), and the copy's slots
    uint32_t n = 0;                // codes held here
    uint32_t global_n = 0;         // codes of the whole partition (== n unless sharded)
    uint32_t first_pos = 0;        // global position of local code 0
    uint32_t start_n = 0;
    uint32_t key_base = 0;
    uint8_t* d_bktw = nullptr;      // 16x4: the wide tiles of the bucket copy (kBktwTileBytes per tile), or null
    uint8_t* d_bktw_side = nullptr; // ... and their side array (kBktSideBytes per tile)
    uint64_t bktw_block = 0;        // W: octave j >= 0 covers positions [W 2^j, W 2^(j+1)) (a power of two, a multiple of bkt_block)
    std::vector<uint64_t> bktw_off; // [octaves + 1] first slot of every octave in the wide copy (multiples of kSplitTile), and its
                                    // slots; an octave without slots fell back to narrow blocks
};

// ... of the index's options (qadc_index has the meaning of each), and of the batch (Slot has them).  Aggregates, in this order.
struct LevelOptions {
    int M;
    uint64_t level_base, level_growth;
    int head_level;
    uint32_t small_run;
    int wgs_per_item, share_variant, mq;
    uint32_t prescan_sample;
    uint64_t split_min_run, split6_min_run;
    uint64_t split5_min_run = 0;   // 0 = never the 5-plane form
    // the nibble form: runs of at least nib8_min_run codes stream 8 of the 16 sub-quantizers, else those of at least nib_min_run
    // stream nib_ns (9 or 10) of them; 0 = never
    uint64_t nib_min_run = 0, nib8_min_run = 0;
    int nib_ns = 9;
    // the bucket form: runs of at least bkt_min_run codes that cover whole blocks of a bucket copy stream 7 of sub-quantizers 4-15,
    // those of at least bkt6_min_run 6, bkt5_min_run 5, bkt4_min_run 4 (the fewest whose threshold the launch's shortest run reaches); 0 = never
    uint64_t bkt_min_run = 0, bkt6_min_run = 0, bkt5_min_run = 0, bkt4_min_run = 0;
    // the wide form: runs of at least bktw_min_run codes that cover whole wide octaves stream 6 of sub-quantizers 5-15, those of at
    // least bktw5_min_run 5, bktw4_min_run 4, bktw3_min_run 3 (as above); 0 = never
    uint64_t bktw_min_run = 0, bktw5_min_run = 0, bktw4_min_run = 0, bktw3_min_run = 0;
};
struct LevelBatch {
    int nq, ma;
    const int32_t* assign;   // [nq][ma]
    int R, mode;
    bool float_path, full_prescan;
    int pre_slice, pre_nslices;
    uint32_t inj_n;
};

// What the planner hands to the launcher: the work items of a batch in upload order.
struct BatchPlan {
    std::string refused;                         // not empty: the batch cannot be planned, and why (nothing below is to be used)
    std::vector<ScanItem> all_items;             // runs, grouped by bound level (launches index into it)
    std::vector<StartItem> sitems_a, sitems_b;   // pre-scan: phase A = unfiltered sample, phase B = filtered remainder
    std::vector<uint32_t> fc_init;               // per query: {sample values, capacity} of its pre-scan buffer
    uint64_t fc_stride = 1;
    std::vector<LevelLaunch> launches;           // kernel and grid of every level launch, in launch order
    uint64_t head_codes = 0;                     // codes of every query's scan order covered by the head launch (0 = none)
    uint64_t start_codes = 0;                    // codes the pre-scan items cover
};

// Level boundaries in the concatenated scan position space of one query.
inline void level_bounds(const LevelOptions& o, uint64_t* L) {
    L[0] = 0;
    uint64_t b = std::max<uint64_t>(o.level_base, 16);
    for (int k = 1; k < kMaxLevels; ++k) {
        L[k] = b;
        b = (b > (UINT64_MAX >> 8)) ? UINT64_MAX : b * std::max<uint64_t>(o.level_growth, 2);
    }
    L[kMaxLevels] = UINT64_MAX;
}

// Workgroups per run (per group of 8 runs: mq) of a level launch, one function per launch class.  maxn = the longest run of the
// launch, nvec = its 16-byte vectors, cnt = the runs of the launch.
inline int wgs_mq(const LevelOptions& o, uint64_t maxn, uint64_t nvec, size_t cnt) {
    // 8 queries per pass (scan_i8_mq_kernel): 256-thread workgroups, ~64 Ki codes each, groups of 8
    // queries as L2-sharing siblings
    const uint64_t tiles = std::max<uint64_t>((nvec + 255) / 256, 1);
    uint64_t w = o.wgs_per_item > 0 ? (uint64_t)o.wgs_per_item
                                    : (maxn + kMqCodesPerWg - 1) / kMqCodesPerWg;
    const uint64_t ngroups = (cnt + 7) / 8;
    w = std::max<uint64_t>(w, (kMqMinWgs + ngroups - 1) / ngroups);   // >= 2 rounds of the 2048 resident workgroups
    w = std::min<uint64_t>(std::min<uint64_t>(w, 65536), std::max<uint64_t>(tiles / kMqMinTiles, 1));
    if (w >= 8) w &= ~7ull;
    return (int)w;
}

inline int wgs_shared(const LevelOptions& o, uint64_t maxn, uint64_t nvec) {
    // Queries of a batch over the same codes (flat database; IVF queries probing the same cell): the
    // sibling-major launch makes them share every tile through one XCD's L2, so the codes cross the
    // HBM interface about once per LAUNCH, not once per query, and the launch is bound by the LDS
    // lookup rate instead.  Workgroups per run: ~2M codes each (amortises the table build, leaves the
    // dispatcher room to balance), a multiple of 8 so that the XCD decode applies.
    uint64_t w = o.wgs_per_item > 0 ? (uint64_t)o.wgs_per_item
                                    : (maxn + kShareCodesPerWg - 1) / kShareCodesPerWg;
    w = std::min<uint64_t>(std::max<uint64_t>(w, 64), 512);
    w = std::min<uint64_t>(w, std::max<uint64_t>((nvec + 4095) / 4096, 1));
    if (w >= 8) w &= ~7ull;
    return (int)w;
}

inline int wgs_small(uint64_t nvec, size_t cnt) {
    // enough workgroups to fill the chip, but no more: each one pays a table build + bound fetch
    const uint64_t want = std::max<uint64_t>(1, 4096 / cnt);
    return (int)std::min<uint64_t>(std::max<uint64_t>((nvec + kSmallVecPerWg - 1) / kSmallVecPerWg, 1), want);
}

inline int wgs_streaming(const LevelOptions& o, uint64_t maxn, uint64_t nvec, size_t cnt, bool split) {
    const int wgs_cap = o.wgs_per_item > 0 ? o.wgs_per_item : (o.M == 16 ? 1024 : 512);   // (r02 sweep: 1024 reaches the streaming ceiling of the "probe" variant, 512 is 1.6 % below)
    // each streaming workgroup builds a 64-128 KiB table: with many runs in the launch, give every
    // workgroup more tiles instead of more workgroups per run (the split form: at least one 16 Ki-code tile each)
    const uint64_t want = std::max<uint64_t>(1, 8192 / cnt);
    const uint64_t units = split ? (maxn + kSplitTile - 1) / kSplitTile : (nvec + 4095) / 4096;
    return (int)std::min<uint64_t>(std::max<uint64_t>(units, 1), std::min<uint64_t>(wgs_cap, want));
}

// May the run [b0, b0 + len) of partition pt take the bucket form?  The partition has the copy, the run starts on a block of it,
// ends on one or at the partition's end, and has at least bkt_min_run codes.
inline bool bkt_run_ok(const LevelPart& pt, const LevelOptions& o, uint64_t b0, uint64_t len) {
    if (!pt.d_bkt || !pt.d_bkt_side || !pt.bkt_block || pt.bkt_off.empty() || o.bkt_min_run == 0 || len < o.bkt_min_run) return false;
    return b0 % pt.bkt_block == 0 && ((b0 + len) % pt.bkt_block == 0 || b0 + len == pt.n);
}
// Paid planes of a bucket launch whose shortest run has minn codes
inline int bkt_planes(const LevelOptions& o, uint64_t minn) {
    return o.bkt4_min_run != 0 && minn >= o.bkt4_min_run ? 4 : o.bkt5_min_run != 0 && minn >= o.bkt5_min_run ? 5
           : o.bkt6_min_run != 0 && minn >= o.bkt6_min_run ? 6 : 7;
}

// The wide octaves of a partition: octave j = 0, 1, ... covers positions [W << j, min(W << (j + 1), n)).
inline size_t bktw_octaves(const LevelPart& pt) { return pt.bktw_off.empty() ? 0 : pt.bktw_off.size() - 1; }
inline bool bktw_is_wide(const LevelPart& pt, size_t j) { return pt.bktw_off[j + 1] > pt.bktw_off[j]; }
// Does [b0, b0 + len) meet an octave that is stored wide?  Such a range has no narrow blocks: no narrow bucket run may cover it.
inline bool bktw_meets(const LevelPart& pt, uint64_t b0, uint64_t len) {
    if (!pt.d_bktw || !pt.bktw_block) return false;
    for (size_t j = 0; j < bktw_octaves(pt); ++j)
        if (bktw_is_wide(pt, j) && b0 < std::min<uint64_t>(pt.bktw_block << (j + 1), pt.n) && b0 + len > (pt.bktw_block << j)) return true;
    return false;
}
// May the run [b0, b0 + len) take the wide form?  It starts on an octave, ends on one or at the partition's end, every octave it
// covers is stored wide, and it has at least bktw_min_run codes.  first / last: the octaves it covers, [first, last).
inline bool bktw_run_ok(const LevelPart& pt, const LevelOptions& o, uint64_t b0, uint64_t len, size_t* first = nullptr, size_t* last = nullptr) {
    if (!pt.d_bktw || !pt.d_bktw_side || !pt.bktw_block || o.bktw_min_run == 0 || len < o.bktw_min_run || len == 0) return false;
    const size_t noct = bktw_octaves(pt);
    size_t j0 = noct, j1 = 0;                                // (not found: j0 >= noct, j1 <= j0)
    for (size_t j = 0; j < noct; ++j) {
        if (b0 == (pt.bktw_block << j)) j0 = j;
        if (b0 + len == std::min<uint64_t>(pt.bktw_block << (j + 1), pt.n)) j1 = j + 1;
    }
    if (j0 >= noct || j1 > noct || j1 <= j0) return false;
    for (size_t j = j0; j < j1; ++j)
        if (!bktw_is_wide(pt, j)) return false;
    if (first) *first = j0;
    if (last) *last = j1;
    return true;
}
// Paid planes of a wide launch whose shortest run has minn codes
inline int bktw_planes(const LevelOptions& o, uint64_t minn) {
    return o.bktw3_min_run != 0 && minn >= o.bktw3_min_run ? 3 : o.bktw4_min_run != 0 && minn >= o.bktw4_min_run ? 4
           : o.bktw5_min_run != 0 && minn >= o.bktw5_min_run ? 5 : 6;
}

// Can some run of a partition with a bucket copy still take the nibble form?  Exact for an index of ONE partition, whose
// scan order always starts at the partition's first code (qadc_index_finalize skips the nibble-plane copy when this says no);
// with more partitions the cuts depend on the probe lists, and the answer is yes.  Follows the cuts of plan_levels.
inline bool nib_still_needed(const LevelPart& pt, const LevelOptions& o, bool only_partition);

// Host planning of one batch: cuts every query's scan order into bound levels, emits the runs (ScanItem) and the
// pre-scan items (StartItem), and decides kernel and grid per level launch.  Part: LevelPart, or a struct derived from it.
template <class Part>
BatchPlan plan_levels(const Part* parts, size_t nparts, const LevelOptions& o, const LevelBatch& b) {
    BatchPlan plan;
    const int cs = o.M / 2, nq = b.nq, ma = b.ma;
    const uint32_t cpl = 16 / cs;
    uint64_t L[kMaxLevels + 1];
    level_bounds(o, L);
    std::vector<std::vector<ScanItem>> per_level(kMaxLevels);
    std::vector<std::vector<const uint8_t*>> per_level_nib(kMaxLevels);   // beside every run: its tile in the nibble-plane copy, or nullptr
    struct BktRun { const uint8_t* tiles; const uint8_t* side; uint64_t slots; };
    std::vector<std::vector<BktRun>> per_level_bkt(kMaxLevels);           // ... and in the bucket copy (tiles == nullptr: the run does not qualify)
    std::vector<std::vector<BktRun>> per_level_bktw(kMaxLevels);          // ... and in its wide tiles
    const int k0 = (b.mode != 1 && o.head_level > 0) ? o.head_level : 0;   // levels < k0 belong to the head launch
    plan.head_codes = k0 ? L[k0] : 0;
    plan.fc_init.assign(2 * (size_t)nq, 0);
    for (int q = 0; q < nq; ++q) {
        uint64_t c = 0;
        uint64_t stotal = 0;
        // the starts of a partition this call pre-scans: all of them, or (mode 1) this rank's slice, cut at
        // multiples of 16 codes so that every slice starts on a 16-byte boundary; (mode 2) none
        auto starts_range = [&](const LevelPart& pt, uint64_t& lo, uint64_t& len) {
            lo = 0;
            len = b.mode == 2 ? 0 : pt.start_n;
            if (b.mode == 1 && b.pre_nslices > 1) {
                lo = ((uint64_t)pt.start_n * b.pre_slice / b.pre_nslices) & ~15ull;
                const uint64_t hi = b.pre_slice + 1 == b.pre_nslices
                                        ? pt.start_n : (((uint64_t)pt.start_n * (b.pre_slice + 1) / b.pre_nslices) & ~15ull);
                len = hi > lo ? hi - lo : 0;
            }
        };
        if (b.float_path)
            for (int a = 0; a < ma; ++a) {
                const int p = b.assign[(size_t)q * ma + a];
                if (p >= 0 && p < (int)nparts) {
                    uint64_t lo, len;
                    starts_range(parts[p], lo, len);
                    stotal += len;
                }
            }
        // two-phase pre-scan only pays (and is only needed) when the starts are many
        uint64_t sample = (b.full_prescan || stotal <= 2ull * o.prescan_sample) ? stotal : o.prescan_sample;
        uint64_t soff = 0;
        for (int a = 0; a < ma; ++a) {
            const int p = b.assign[(size_t)q * ma + a];
            if (p < 0 || p >= (int)nparts) {
                plan.refused = "assign[] names a partition that does not exist";
                return plan;
            }
            const LevelPart& pt = parts[p];
            if (pt.global_n == 0) continue;  // empty partition: db_query_4.cpp:291-293
            uint64_t slo = 0, slen = 0;
            if (b.float_path) starts_range(pt, slo, slen);
            if (slen) {
                const uint8_t* sc = (pt.d_starts ? pt.d_starts : pt.d_codes) + slo * cs;
                const uint64_t in_a = soff < sample ? std::min<uint64_t>(slen, sample - soff) : 0;
                StartItem si;
                si.table = (uint32_t)((size_t)q * ma + a);
                si.query = (uint32_t)q;
                if (in_a) {
                    si.codes = sc;
                    si.n = (uint32_t)in_a;
                    si.out_off = (uint32_t)soff;
                    si.filter = 0;
                    plan.sitems_a.push_back(si);
                }
                if (in_a < slen) {
                    si.codes = sc + in_a * cs;
                    si.n = (uint32_t)(slen - in_a);
                    si.out_off = 0;
                    si.filter = 1;
                    plan.sitems_b.push_back(si);
                }
                soff += slen;
                plan.start_codes += slen;
            }
            if (pt.n == 0 || b.mode == 1) continue;   // no codes of the partition here (only its starts replica) / pre-scan only
            uint64_t prev = 0;
            for (int k = 0; k < kMaxLevels && prev < pt.n; ++k) {
                uint64_t cut = pt.n;
                if (L[k + 1] < c + pt.n) {
                    cut = L[k + 1] > c ? L[k + 1] - c : 0;
                    cut -= cut % cpl;  // keep every run 16-byte aligned
                }
                if (cut <= prev) continue;
                if (k < k0) {                                 // scanned by the head launch (same cut: scan_query_kernel, HEAD)
                    prev = cut;
                    continue;
                }
                // runs longer than 2^31 codes are cut so that 32-bit vector indices cannot wrap
                for (uint64_t b0 = prev; b0 < cut;) {
                    const uint64_t len = std::min<uint64_t>(cut - b0, 1ull << 31);
                    ScanItem it;
                    it.codes = pt.d_codes + b0 * cs;
                    it.labels = pt.d_labels;
                    it.n = (uint32_t)len;
                    it.pos0 = (uint32_t)b0;
                    it.key_base = pt.key_base + pt.first_pos;
                    it.table = (uint32_t)((size_t)q * ma + a);
                    it.query = (uint32_t)q;
                    it.order = ((uint32_t)k << 16) | (uint32_t)a;
                    // padding-lane replay of the partition's last code (simd_layout.hpp:46-50, simd_scan.hpp:67)
                    it.dup_pos = (pt.first_pos + pt.n == pt.global_n) ? pt.n - 1u : 0xffffffffu;
                    it.dup_reps = (16u - pt.global_n % 16u) % 16u;
                    // a long run that starts on a tile of the partition's byte-plane copy may take the split form
                    it.split = pt.d_split && b0 % kSplitTile == 0 && len >= std::max<uint64_t>(o.split_min_run, o.small_run)
                                   ? pt.d_split + b0 / kSplitTile * (uint64_t)kSplitBytes * kSplitTile : nullptr;
                    // ... and, where the partition has a nibble-plane copy as well, the nibble form (same tiles)
                    per_level_nib[k].push_back(it.split && pt.d_nib ? pt.d_nib + b0 / kSplitTile * (uint64_t)kNibTileBytes : nullptr);
                    BktRun br{nullptr, nullptr, 0};
                    BktRun bw{nullptr, nullptr, 0};
                    size_t oc0 = 0, oc1 = 0;
                    if (it.split && bktw_run_ok(pt, o, b0, len, &oc0, &oc1)) {
                        const uint64_t s0 = pt.bktw_off[oc0], s1 = pt.bktw_off[oc1];
                        if (s1 - s0 <= 0xffffffffull && s0 % kSplitTile == 0 && s1 % kSplitTile == 0)
                            bw = BktRun{pt.d_bktw + s0 / kSplitTile * (uint64_t)kBktwTileBytes,
                                        pt.d_bktw_side + s0 / kSplitTile * (uint64_t)kBktSideBytes, s1 - s0};
                    }
                    per_level_bktw[k].push_back(bw);
                    if (it.split && bkt_run_ok(pt, o, b0, len) && !bktw_meets(pt, b0, len)) {
                        const size_t blk0 = (size_t)(b0 / pt.bkt_block);
                        const size_t blk1 = std::min<size_t>((size_t)((b0 + len + pt.bkt_block - 1) / pt.bkt_block), pt.bkt_off.size() - 1);
                        const uint64_t s0 = pt.bkt_off[blk0], s1 = pt.bkt_off[blk1];
                        if (blk1 > blk0 && s1 > s0 && s1 - s0 <= 0xffffffffull && s0 % kSplitTile == 0 && s1 % kSplitTile == 0)
                            br = BktRun{pt.d_bkt + s0 / kSplitTile * (uint64_t)kBktTileBytes,
                                        pt.d_bkt_side + s0 / kSplitTile * (uint64_t)kBktSideBytes, s1 - s0};
                    }
                    per_level_bkt[k].push_back(br);
                    per_level[k].push_back(it);
                    b0 += len;
                }
                prev = cut;
            }
            c += pt.n;
        }
        // survivors of the filter: expected R * stotal / sample; 16x head-room, the overflow flag catches the rest
        uint64_t cap = sample;
        if (sample < stotal)
            cap += std::min<uint64_t>(stotal - sample, std::max<uint64_t>(16ull * b.R * ((stotal + sample - 1) / sample), 4096));
        if (b.mode == 2) sample = cap = b.inj_n;              // the gathered values are the whole "pre-scan output"
        plan.fc_init[2 * q] = (uint32_t)sample;
        plan.fc_init[2 * q + 1] = (uint32_t)cap;
        plan.fc_stride = std::max<uint64_t>(plan.fc_stride, cap);
    }
    size_t nitems = 0;
    for (auto& v : per_level) nitems += v.size();
    plan.all_items.assign(nitems, ScanItem());
    size_t off = 0;
    for (int k = 0; k < kMaxLevels; ++k) {
        if (per_level[k].empty()) continue;
        // one launch for the short runs of the level, one for the long ones (one more for those of them with a byte-plane copy)
        for (int cls = 0; cls < 3; ++cls) {
            const int small = cls == 0 ? 1 : 0;
            uint64_t maxn = 0, minn = ~0ull, codes = 0;
            size_t cnt = 0;
            bool same = true, all_nib = true, all_bkt = true, all_bktw = true;
            std::vector<const uint8_t*> nibs;
            std::vector<BktRun> bkts, bktws;
            for (size_t r = 0; r < per_level[k].size(); ++r) {
                const ScanItem& it = per_level[k][r];
                if ((it.n < o.small_run) != (small == 1)) continue;
                if (!small && (it.split != nullptr) != (cls == 2)) continue;
                if (cnt) {
                    const ScanItem& f = plan.all_items[off];
                    same = same && it.codes == f.codes && it.n == f.n && it.pos0 == f.pos0 && it.labels == f.labels &&
                           it.key_base == f.key_base && it.dup_pos == f.dup_pos && it.dup_reps == f.dup_reps;
                }
                plan.all_items[off + cnt++] = it;
                maxn = std::max<uint64_t>(maxn, it.n);
                minn = std::min<uint64_t>(minn, it.n);
                codes += it.n;
                all_nib = all_nib && per_level_nib[k][r] != nullptr;
                nibs.push_back(per_level_nib[k][r]);
                all_bkt = all_bkt && per_level_bkt[k][r].tiles != nullptr;
                bkts.push_back(per_level_bkt[k][r]);
                all_bktw = all_bktw && per_level_bktw[k][r].tiles != nullptr;
                bktws.push_back(per_level_bktw[k][r]);
            }
            if (!cnt) continue;
            const uint64_t nvec = (maxn + cpl - 1) / cpl;
            LevelLaunch ll;
            ll.first = off;
            ll.nitems = (int)cnt;
            ll.small = small == 1;
            ll.maxn = maxn;
            ll.early = false;
            ll.shared = !ll.small && same && cnt >= 2 && o.share_variant != 0;
            ll.mq = ll.shared && o.mq;
            ll.split = cls == 2 && !ll.shared;
            ll.split6 = ll.split && o.split6_min_run != 0 && minn >= o.split6_min_run;
            ll.split5 = ll.split && o.split5_min_run != 0 && minn >= o.split5_min_run;
            ll.nib = !(ll.split && all_nib)                              ? 0
                     : o.nib8_min_run != 0 && minn >= o.nib8_min_run    ? 8
                     : o.nib_min_run != 0 && minn >= o.nib_min_run      ? (o.nib_ns == 10 ? 10 : 9)
                                                                        : 0;
            ll.bktw = ll.split && all_bktw ? bktw_planes(o, minn) : 0;
            ll.bkt = ll.split && all_bkt && !ll.bktw ? bkt_planes(o, minn) : 0;
            uint64_t max_slots = 0;
            if (ll.bktw) bkts.swap(bktws);                               // the launch reads the wide tiles: the same bookkeeping
            if (ll.bkt || ll.bktw) {                                                // the launch reads the bucket copy: its runs count slots
                ll.nib = 0;
                for (size_t r = 0; r < cnt; ++r) {
                    ScanItem& it = plan.all_items[off + r];
                    it.split = bkts[r].tiles;
                    it.codes = bkts[r].side;
                    it.n = (uint32_t)bkts[r].slots;
                    max_slots = std::max(max_slots, bkts[r].slots);
                    ll.slots += bkts[r].slots;
                }
            }
            if (ll.nib)                                                  // the launch reads the nibble-plane copy instead
                for (size_t r = 0; r < cnt; ++r) plan.all_items[off + r].split = nibs[r];
            ll.wgs = ll.mq       ? wgs_mq(o, maxn, nvec, cnt)
                     : ll.shared ? wgs_shared(o, maxn, nvec)
                     : ll.small  ? wgs_small(nvec, cnt)
                     : ll.bkt || ll.bktw ? wgs_streaming(o, max_slots, (max_slots + cpl - 1) / cpl, cnt, true)
                                 : wgs_streaming(o, maxn, nvec, cnt, ll.split);
            ll.codes = codes;
            plan.launches.push_back(ll);
            off += cnt;
        }
    }
    return plan;
}

inline bool nib_still_needed(const LevelPart& pt, const LevelOptions& o, bool only_partition) {
    if (!pt.d_bkt || !only_partition) return true;
    const uint64_t nib_min = o.nib_min_run && o.nib8_min_run ? std::min(o.nib_min_run, o.nib8_min_run) : std::max(o.nib_min_run, o.nib8_min_run);
    if (nib_min == 0) return false;
    const uint32_t cpl = 16 / (o.M / 2);
    uint64_t L[kMaxLevels + 1];
    level_bounds(o, L);
    uint64_t prev = 0;
    for (int k = 0; k < kMaxLevels && prev < pt.n; ++k) {
        uint64_t cut = pt.n;
        if (L[k + 1] < pt.n) cut = L[k + 1] - L[k + 1] % cpl;
        if (cut <= prev) continue;
        for (uint64_t b0 = prev; b0 < cut;) {
            const uint64_t len = std::min<uint64_t>(cut - b0, 1ull << 31);
            if (len >= std::max<uint64_t>(nib_min, std::max<uint64_t>(o.split_min_run, o.small_run)) && b0 % kSplitTile == 0 &&
                !(bkt_run_ok(pt, o, b0, len) && !bktw_meets(pt, b0, len)) && !bktw_run_ok(pt, o, b0, len))
                return true;
            b0 += len;
        }
        prev = cut;
    }
    return false;
}

}  // namespace host
}  // namespace qadc
