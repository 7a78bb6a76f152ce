// CPU driver of the append path's refusals (host/append_check.hpp; tests/test_append_check_host.py): one check per run, the status
// and the text on stdout as "<status>\n<text>\n".  No HIP, no library.
//   add <call> <set_pq> <dim> <K> <max_dim> <labeled> <sizes: a,b,... or -> <labelled> <has_vectors> <has_labels> <count>
//       <labels_offset> <sum_mode>
//   reserve <part_count> <has_capacities>
//   read <sizes> <part> <first> <count>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../quick-adc_amd/host/append_check.hpp"

using namespace qadc::adc;

static std::vector<uint32_t> list(const std::string& s) {
    std::vector<uint32_t> v;
    if (s == "-") return v;
    size_t at = 0;
    while (at <= s.size()) {
        const size_t comma = std::min(s.find(',', at), s.size());
        v.push_back((uint32_t)std::strtoull(s.substr(at, comma - at).c_str(), nullptr, 10));
        at = comma + 1;
    }
    return v;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    AppendRefusal r;
    if (mode == "add" && argc == 15) {
        const std::vector<uint32_t> sizes = list(argv[8]);
        AppendCall c;
        c.call = argv[2];
        c.set_pq = argv[3];
        c.dim = std::atoi(argv[4]);
        c.K = std::atoi(argv[5]);
        c.max_dim = std::atoi(argv[6]);
        c.labeled = std::atoi(argv[7]);
        c.sizes = sizes.data();
        c.parts = sizes.size();
        c.labelled = std::atoi(argv[9]) != 0;
        c.has_vectors = std::atoi(argv[10]) != 0;
        c.has_labels = std::atoi(argv[11]) != 0;
        c.count = std::strtoull(argv[12], nullptr, 10);
        c.labels_offset = (uint32_t)std::strtoull(argv[13], nullptr, 10);
        c.sum_mode = std::atoi(argv[14]);
        r = check_add_vectors(c);
    } else if (mode == "reserve" && argc == 4) {
        r = check_reserve(std::atoi(argv[2]), std::atoi(argv[3]) != 0);
    } else if (mode == "read" && argc == 6) {
        const std::vector<uint32_t> sizes = list(argv[2]);
        r = check_read_partition(sizes.data(), sizes.size(), std::atoi(argv[3]), (uint32_t)std::strtoull(argv[4], nullptr, 10),
                                 (uint32_t)std::strtoull(argv[5], nullptr, 10));
    } else {
        return 2;
    }
    printf("%d\n%s\n", r.status, r.text.c_str());
    return 0;
}
