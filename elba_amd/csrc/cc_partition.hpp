// cc_partition.hpp — the greedy assignment of components to parts that elba_partition_components runs on the host between the labelling
// and the gather kernel (components.hip; the rule is stated in include/elba_amd.h).  It is the loop of the reference's GetContigSizes /
// GetLocalProcAssignments (src/ContigGeneration.cpp:126, :184-197) with its two open ends closed: ties of the sort go to the smaller
// component number, ties of the minimum to the lower part index.  Plain C++17, no HIP: the list of components is small, and
// elba_amd/hostcpp/test_cc_partition.cpp compiles this file alone under the sanitizers.
#pragma once
#include <algorithm>
#include <cstdint>
#include <functional>
#include <queue>
#include <utility>
#include <vector>

namespace elba {

// reads[c], weight[c] of the n components (weight >= 0); nparts >= 1.  part_of_comp[c] = the part of component c, -1 when reads[c] <
// min_reads; part_weight[p] = the sum of the weights dealt to part p.  The parts wait in a heap ordered by (sum, index), whose top is what
// std::min_element returns on the array of sums: n log nparts steps however many parts there are.
inline void cc_partition(const int64_t *reads, const int64_t *weight, int64_t n, int32_t nparts, int64_t min_reads, std::vector<int32_t> &part_of_comp,
                         std::vector<int64_t> &part_weight)
{
    part_of_comp.assign((size_t)n, -1);
    part_weight.assign((size_t)nparts, 0);
    std::vector<int64_t> order;
    for (int64_t c = 0; c < n; ++c) if (reads[c] >= min_reads) order.push_back(c);
    std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return weight[a] > weight[b]; });      // (stable over ascending numbers: the tie rule)
    using Part = std::pair<int64_t, int32_t>;      // (sum so far, index)
    std::priority_queue<Part, std::vector<Part>, std::greater<Part>> parts;
    for (int32_t p = 0; p < nparts; ++p) parts.push({0, p});
    for (const int64_t c : order) {
        const Part t = parts.top();
        parts.pop();
        part_of_comp[(size_t)c] = t.second;
        part_weight[(size_t)t.second] = t.first + weight[c];
        parts.push({t.first + weight[c], t.second});
    }
}

}  // namespace elba
