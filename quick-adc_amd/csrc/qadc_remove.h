// Remove by label: the flow both engines share — qadc_adc_index_remove_labels (csrc/qadc_adc.cpp) over the
// regions of the owned float-ADC database, qadc_index_remove_labels (csrc/qadc_index_add.cpp) over the partitions of a 4-bit
// index, in the arena or not.  Internal header; the kernels are in csrc/qadc_adc_kernel.hip, the decisions in host/remove_plan.hpp.
//
//   1. mark     (mark_list, which the key filters of the float-ADC scan share) the list is uploaded (host form) or read where it lies (device form, whose lo / hi come from remove_minmax_kernel
//               and one synchronise of their own: the bitmap cannot be sized before them); a bitmap over [lo, hi] is allocated
//               for the call, zeroed on the stream and filled by remove_mark_kernel;
//   2. count    remove_count_kernel reads every label once; hits[] and first[] come back in one pinned copy — the call's only
//               download (the device form's two words of step 1 apart).  No partition hit: the call ends here, nothing written;
//   3. compact  one workgroup per touched partition moves the kept rows to the front (remove_compact_kernel) and, for the 4-bit
//               index, zeroes the bytes behind the new last row.
// Every copy and memset is the Async form on the caller's stream; the call is synchronous (it returns after the stream drained).
#pragma once
#include "../host/remove_plan.hpp"
#include "qadc_adc_kernels.h"
#include "qadc_host.h"

namespace qadc {
namespace host {

struct RemoveJob {
    hipStream_t stream = nullptr;
    int code_size = 0;                      // 4, 8 or 16 bytes a row
    bool zero_tail = false;                 // the 4-bit index: bytes [n' * cs, align16(n' * cs) + 64) behind the new end are zeroed
    std::vector<uint8_t*> codes;            // [parts] where every partition's rows lie (anything for an empty one)
    std::vector<uint32_t*> labels;          // [parts] ... and its labels
    std::vector<uint32_t> sizes;            // [parts] rows held
    PinBuf<uint32_t>* pinned = nullptr;     // the index's pinned staging block (grown as needed)
    // results
    adc::RemovePlan plan;                   // plan.sizes: what the caller commits after QADC_OK
    bool wrote = false;                     // the compaction was enqueued: after a failure the touched partitions are unspecified
};

// Step 1, shared with the key filters of the float-ADC scan (qadc_adc_filter_create*, csrc/qadc_adc.cpp): the bitmap of a list of
// `count` > 0 keys in host memory, or (d_side) in device memory, read by kernels only.  Everything is enqueued on `s`; the device
// form synchronises once for lo / hi.  `tmp` takes what only the call needs (the uploaded list, the two words of lo / hi) and must
// outlive the stream's work; `own` takes the bitmap (span->words words), which the caller keeps as long as it tests keys with it.
// pinned: a staging block for the two words of the device form.
inline int mark_list(hipStream_t s, const uint32_t* list, uint64_t count, bool d_side, PinBuf<uint32_t>* pinned, Scratch& tmp, Scratch& own,
                     adc::RemoveSpan* span, uint32_t** d_bitmap) {
    using namespace qadc::adc;
    uint32_t lo = 0xffffffffu, hi = 0;
    const uint32_t* d_list = list;
    if (d_side) {
        uint32_t* d_lohi = nullptr;
        HIPCHECK(pinned->ensure(2));
        HIPCHECK(tmp.alloc(&d_lohi, 8));
        HIPCHECK(hipMemsetAsync(d_lohi, 0xff, 4, s));
        HIPCHECK(hipMemsetAsync(d_lohi + 1, 0, 4, s));
        HIPCHECK(launch_remove_minmax(list, count, d_lohi, s));
        HIPCHECK(hipMemcpyAsync(pinned->p, d_lohi, 8, hipMemcpyDeviceToHost, s));
        HIPCHECK(hipStreamSynchronize(s));
        lo = pinned->p[0];
        hi = pinned->p[1];
    } else {
        for (uint64_t i = 0; i < count; ++i) {
            lo = std::min(lo, list[i]);
            hi = std::max(hi, list[i]);
        }
        uint32_t* d_up = nullptr;
        HIPCHECK(tmp.alloc(&d_up, count * 4));
        HIPCHECK(hipMemcpyAsync(d_up, list, count * 4, hipMemcpyHostToDevice, s));
        d_list = d_up;
    }
    *span = remove_span(lo, hi);
    HIPCHECK(own.alloc(d_bitmap, span->words * 4));
    HIPCHECK(hipMemsetAsync(*d_bitmap, 0, span->words * 4, s));
    HIPCHECK(launch_remove_mark(d_list, count, span->lo, *d_bitmap, s));
    return QADC_OK;
}

// list: `count` > 0 labels in host memory, or (d_side) in device memory, read by kernels only.
inline int remove_rows(RemoveJob& job, const uint32_t* list, uint64_t count, bool d_side) {
    using namespace qadc::adc;
    const size_t parts = job.sizes.size();
    hipStream_t s = job.stream;
    Scratch mem;
    HIPCHECK(job.pinned->ensure(std::max<size_t>(2 * parts, 2)));
    RemoveSpan span;
    uint32_t* d_bitmap = nullptr;
    if (int rc = mark_list(s, list, count, d_side, job.pinned, mem, mem, &span, &d_bitmap)) return rc;

    std::vector<RemoveSrc> src(parts);
    uint32_t longest = 0;
    for (size_t p = 0; p < parts; ++p) {
        src[p] = RemoveSrc{job.sizes[p] ? job.labels[p] : nullptr, job.sizes[p], 0};
        longest = std::max(longest, job.sizes[p]);
    }
    RemoveSrc* d_src = nullptr;
    uint32_t* d_stat = nullptr;   // [hits parts | first parts]
    HIPCHECK(mem.alloc(&d_src, parts * sizeof(RemoveSrc)));
    HIPCHECK(mem.alloc(&d_stat, 2 * parts * 4));
    HIPCHECK(hipMemcpyAsync(d_src, src.data(), parts * sizeof(RemoveSrc), hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemsetAsync(d_stat, 0, parts * 4, s));
    HIPCHECK(hipMemsetAsync(d_stat + parts, 0xff, parts * 4, s));
    HIPCHECK(launch_remove_count(d_src, (int)parts, longest, d_bitmap, span.lo, span.last, d_stat, d_stat + parts, s));
    HIPCHECK(hipMemcpyAsync(job.pinned->p, d_stat, 2 * parts * 4, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));

    job.plan = plan_remove(job.code_size, parts, job.sizes.data(), job.pinned->p, job.pinned->p + parts, (uint32_t)kRemoveTile, job.zero_tail);
    const size_t touched = job.plan.touched.size();
    if (touched == 0) return QADC_OK;

    std::vector<RemovePart> table(touched);
    for (size_t i = 0; i < touched; ++i) {
        const RemoveEntry& e = job.plan.touched[i];
        table[i] = RemovePart{job.codes[e.part], job.labels[e.part], e.n, e.first_tile, (uint32_t)(e.zero_last - e.zero_first), 0};
    }
    RemovePart* d_table = nullptr;
    HIPCHECK(mem.alloc(&d_table, touched * sizeof(RemovePart)));
    HIPCHECK(hipMemcpyAsync(d_table, table.data(), touched * sizeof(RemovePart), hipMemcpyHostToDevice, s));
    job.wrote = true;
    HIPCHECK(launch_remove_compact(d_table, (uint32_t)touched, job.code_size, d_bitmap, span.lo, span.last, s));
    HIPCHECK(hipStreamSynchronize(s));
    return QADC_OK;
}

}  // namespace host
}  // namespace qadc
