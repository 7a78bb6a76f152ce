// The refusals of the append path: what qadc_index_add_vectors* / qadc_adc_index_add_vectors*, _reserve and
// _read_partition refuse before the device is touched, as pure functions over what the engine knows of its index.  No HIP:
// csrc/qadc_append.h runs them for both engines, and tests/cpp/append_check_host.cpp drives every refusal on a CPU.  What depends on
// engine-private state (busy slots, views, shards, borrowed partitions) is refused by the engine before these.
#pragma once
#include <cstdint>
#include <string>

#include "../../include/qadc.h"
#include "adc_append_plan.hpp"

namespace qadc {
namespace adc {

struct AppendRefusal {
    int status = QADC_OK;         // QADC_E_ARG or QADC_E_STATE with the text of qadc_last_error
    std::string text;
};

// One add_vectors call as the checks see it.
struct AppendCall {
    const char* call = "";          // the entry point's name
    const char* set_pq = "";        // the engine's qadc_*_set_pq, named where the index has no codebooks
    int dim = 0, K = 0;             // the quantizers the index holds (dim 0: none; K 0: flat)
    int max_dim = 0;                // the widest vector the engine's encoder takes (0: any)
    int labeled = -1;               // -1 unknown, 0 keyed by position, 1 labelled
    const uint32_t* sizes = nullptr;   // [parts] rows every partition holds
    size_t parts = 0;
    bool labelled = false;          // the call takes labels [count] and no labels_offset
    bool has_vectors = false, has_labels = false;   // the pointers are not null
    uint64_t count = 0;
    uint32_t labels_offset = 0;
    int sum_mode = 1;
};

inline AppendRefusal append_refuse(int status, const std::string& text) {
    AppendRefusal r;
    r.status = status;
    r.text = text;
    return r;
}

inline AppendRefusal check_add_vectors(const AppendCall& c) {
    bool holds = false;
    for (size_t p = 0; p < c.parts; ++p) holds = holds || c.sizes[p] != 0;
    const std::string call = c.call;
    if (c.labelled) {   // (the keys of a flat or unlabelled index are positions: it has no label to set)
        if (c.dim && !c.K)
            return append_refuse(QADC_E_STATE, call + ": a flat index (no coarse quantizer) keys its vectors by position and takes no labels");
        if (c.labeled == 0 && holds) return append_refuse(QADC_E_STATE, call + ": the index holds unlabelled partitions, whose keys are positions");
        if (c.count && !c.has_labels) return append_refuse(QADC_E_ARG, "labels is null");
    }
    if (!c.dim) return append_refuse(QADC_E_ARG, std::string(c.set_pq) + " has not been called: the index has no codebooks");
    if (c.max_dim && c.dim > c.max_dim)
        return append_refuse(QADC_E_ARG, "dim must be <= " + std::to_string(c.max_dim) + " (the encoder keeps the codebooks in LDS)");
    if (c.sum_mode != 0 && c.sum_mode != 1) return append_refuse(QADC_E_ARG, "sum_mode is 0 (source order) or 1 (as compiled)");
    if (c.count && !c.has_vectors) return append_refuse(QADC_E_ARG, "vectors is null");
    if ((uint64_t)c.labels_offset + c.count > kAppendMaxRows)
        return append_refuse(QADC_E_ARG, "labels_offset + count = " + std::to_string((uint64_t)c.labels_offset + c.count) + " exceeds 2^32 - 1");
    if (c.K) {
        if (c.parts != 0 && c.parts != (size_t)c.K)
            return append_refuse(QADC_E_ARG, "the coarse quantizer has " + std::to_string(c.K) + " centroids and the index " + std::to_string(c.parts) +
                                                 " partitions");
        if (c.labeled == 0 && holds)
            return append_refuse(QADC_E_ARG, "the index holds unlabelled partitions: vectors added through a coarse quantizer are labelled");
    } else {
        if (c.parts > 1)
            return append_refuse(QADC_E_ARG, "a flat index (no coarse quantizer) has one partition: the index has " + std::to_string(c.parts));
        if (c.labeled == 1 && holds) return append_refuse(QADC_E_ARG, "the index is labelled: a flat index keys its vectors by position");
    }
    return AppendRefusal();
}

inline AppendRefusal check_reserve(int part_count, bool has_capacities) {
    if (part_count < 0 || (part_count > 0 && !has_capacities)) return append_refuse(QADC_E_ARG, "bad capacity array");
    return AppendRefusal();
}

// sizes [parts]: the rows every partition holds.
inline AppendRefusal check_read_partition(const uint32_t* sizes, size_t parts, int part, uint32_t first, uint32_t count) {
    if (part < 0 || part >= (int)parts)
        return append_refuse(QADC_E_ARG, "partition " + std::to_string(part) + " does not exist (" + std::to_string(parts) + " partitions)");
    if ((uint64_t)first + count > sizes[part])
        return append_refuse(QADC_E_ARG, "rows [" + std::to_string(first) + ", " + std::to_string((uint64_t)first + count) + ") are outside partition " +
                                             std::to_string(part) + " of " + std::to_string(sizes[part]) + " codes");
    return AppendRefusal();
}

}  // namespace adc
}  // namespace qadc
