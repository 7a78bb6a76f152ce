// TEST DRIVER (CPU only): the range planner of the float-ADC engine (host/adc_plan.hpp: plan_range, plan_range_rerun, range_entries;
// DESIGN.md section 11.13) printed for tests/test_adc_range_plan_host.py.  C++14, header only, no HIP.
//   usage: adc_range_plan_host IN
//   IN : int32 nparts, nq, ma, has_counts | uint32 sizes [nparts] | int32 assign [nq][ma] | uint64 max_entries
//        | (has_counts) uint32 counts [nq]
//   stdout, one line each:
//        refused <text>                      and nothing more, when plan_range refuses
//        total <nq values> | cap <nq values> | first <entries> <refusal text or ->
//        item <query> <slot> <start> <count> <sbase>        per run
//        (has_counts) rerun <0|1> | recap <nq values> | second <entries> <refusal text or ->
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <vector>

#include "../../quick-adc_amd/host/adc_plan.hpp"

using namespace qadc::adc;

template <typename T>
static void read_vec(std::FILE* f, std::vector<T>& v, std::size_t n) {
    v.resize(n);
    if (n && std::fread(v.data(), sizeof(T), n, f) != n) {
        std::cerr << "short input" << std::endl;
        std::exit(2);
    }
}

template <typename T>
static void line(const char* name, const std::vector<T>& v) {
    std::cout << name;
    for (const T& x : v) std::cout << ' ' << (unsigned long long)x;
    std::cout << '\n';
}

int main(int argc, char** argv) {
    if (argc != 2) {
        std::cerr << "usage: adc_range_plan_host IN" << std::endl;
        return 2;
    }
    std::FILE* in = std::fopen(argv[1], "rb");
    if (!in) return 2;
    std::vector<std::int32_t> head, assign;
    std::vector<std::uint32_t> sizes, counts;
    std::vector<std::uint64_t> max_entries;
    read_vec(in, head, 4);
    const int nparts = head[0], nq = head[1], ma = head[2], has_counts = head[3];
    read_vec(in, sizes, nparts);
    read_vec(in, assign, (std::size_t)nq * ma);
    read_vec(in, max_entries, 1);
    if (has_counts) read_vec(in, counts, nq);
    std::fclose(in);

    Plan p = plan_range(sizes.data(), nq, ma, assign.data());
    if (!p.refused.empty()) {
        std::cout << "refused " << p.refused << std::endl;
        return 0;
    }
    if (p.levels() != 1 || p.level_first.size() != 2 || p.level_first[0] != 0 || p.level_first[1] != p.items.size()) {
        std::cerr << "a range plan has one level over all its items" << std::endl;
        return 1;
    }
    line("total", p.total);
    line("cap", p.cap);
    std::uint64_t entries = 0;
    std::string over = range_entries(p.cap, max_entries[0], &entries);
    std::cout << "first " << entries << ' ' << (over.empty() ? "-" : over) << '\n';
    for (const Item& it : p.items)
        std::cout << "item " << it.query << ' ' << it.slot << ' ' << it.start << ' ' << it.count << ' ' << it.sbase << '\n';
    if (has_counts) {
        std::cout << "rerun " << (plan_range_rerun(p, counts.data()) ? 1 : 0) << '\n';
        line("recap", p.cap);
        over = range_entries(p.cap, max_entries[0], &entries);
        std::cout << "second " << entries << ' ' << (over.empty() ? "-" : over) << '\n';
    }
    std::cout.flush();
    return 0;
}
