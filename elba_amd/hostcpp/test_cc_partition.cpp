// test_cc_partition — walks csrc/cc_partition.hpp without the library: the greedy assignment of components to parts on named cases and on
// a few thousand random ones, against the loop written out as the reference has it (a sort by weight, std::min_element over the array of
// sums), the two tie rules, and the guarantee of the rule (max - min of the sums is at most the largest weight dealt).
// Without arguments it prints one line per failed check and "ok <checks>" at the end (tests/test_cc_partition_cpu.py reads it); exit
// status 1 if a check failed.  With `NPARTS MIN_READS` it reads "reads weight" lines from standard input and prints the part of every
// component on one line and the sums on the next.
#include "../csrc/cc_partition.hpp"
#include <cstdio>
#include <cstdlib>
#include <random>

using namespace elba;

static int g_checks = 0, g_failed = 0;
#define CHECK(cond, ...) do { ++g_checks; if (!(cond)) { ++g_failed; printf("FAILED %s:%d %s | ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } while (0)

// the loop as the reference states it, ties closed as the header says
static void literal(const std::vector<int64_t> &reads, const std::vector<int64_t> &weight, int nparts, int64_t min_reads, std::vector<int32_t> &poc, std::vector<int64_t> &sums)
{
    std::vector<std::pair<int64_t, int64_t>> result;      // (component, weight)
    for (size_t c = 0; c < reads.size(); ++c) if (reads[c] >= min_reads) result.emplace_back((int64_t)c, weight[c]);
    std::sort(result.begin(), result.end(), [](const auto &a, const auto &b) { return a.second != b.second ? a.second > b.second : a.first < b.first; });
    poc.assign(reads.size(), -1);
    sums.assign((size_t)nparts, 0);
    for (const auto &t : result) {
        const size_t where = (size_t)std::distance(sums.begin(), std::min_element(sums.begin(), sums.end()));
        sums[where] += t.second;
        poc[(size_t)t.first] = (int32_t)where;
    }
}

static void check_one(const std::vector<int64_t> &reads, const std::vector<int64_t> &weight, int nparts, int64_t min_reads, const char *what)
{
    std::vector<int32_t> poc, want;
    std::vector<int64_t> pw, sums;
    cc_partition(reads.data(), weight.data(), (int64_t)reads.size(), nparts, min_reads, poc, pw);
    literal(reads, weight, nparts, min_reads, want, sums);
    CHECK(poc == want, "%s: parts differ from the literal loop", what);
    CHECK(pw == sums, "%s: sums differ from the literal loop", what);
    int64_t largest = 0, total = 0;
    std::vector<int64_t> again((size_t)nparts, 0);
    for (size_t c = 0; c < reads.size(); ++c) {
        CHECK((poc[c] >= 0) == (reads[c] >= min_reads), "%s: component %zu", what, c);
        CHECK(poc[c] < nparts, "%s: component %zu names part %d", what, c, (int)poc[c]);
        if (poc[c] >= 0) { again[(size_t)poc[c]] += weight[c]; total += weight[c]; if (weight[c] > largest) largest = weight[c]; }
    }
    CHECK(again == pw, "%s: the sums are not those of the parts", what);
    const auto mm = std::minmax_element(pw.begin(), pw.end());
    CHECK(*mm.second - *mm.first <= largest, "%s: max - min = %lld > largest weight %lld", what, (long long)(*mm.second - *mm.first), (long long)largest);
}

int main(int argc, char **argv)
{
    if (argc == 3) {
        std::vector<int64_t> reads, weight;
        long long r, w;
        while (scanf("%lld %lld", &r, &w) == 2) { reads.push_back(r); weight.push_back(w); }
        std::vector<int32_t> poc;
        std::vector<int64_t> pw;
        cc_partition(reads.data(), weight.data(), (int64_t)reads.size(), std::atoi(argv[1]), std::atoll(argv[2]), poc, pw);
        for (size_t c = 0; c < poc.size(); ++c) printf("%d%s", (int)poc[c], c + 1 < poc.size() ? " " : "");
        printf("\n");
        for (size_t p = 0; p < pw.size(); ++p) printf("%lld%s", (long long)pw[p], p + 1 < pw.size() ? " " : "");
        printf("\n");
        return 0;
    }
    {   // no component at all, and none large enough
        std::vector<int32_t> poc; std::vector<int64_t> pw;
        cc_partition(nullptr, nullptr, 0, 3, 2, poc, pw);
        CHECK(poc.empty() && pw == std::vector<int64_t>({0, 0, 0}), "empty");
        check_one({1, 1, 1}, {1, 1, 1}, 2, 2, "lone reads only");
    }
    {   // equal weights: the tie rules decide — components in ascending order, parts round robin
        std::vector<int32_t> poc; std::vector<int64_t> pw;
        const std::vector<int64_t> r(7, 5);
        cc_partition(r.data(), r.data(), 7, 3, 2, poc, pw);
        CHECK(poc == std::vector<int32_t>({0, 1, 2, 0, 1, 2, 0}), "equal weights");
        CHECK(pw == std::vector<int64_t>({15, 10, 10}), "equal weights: sums");
    }
    {   // the largest first; more parts than components
        std::vector<int32_t> poc; std::vector<int64_t> pw;
        const std::vector<int64_t> r = {2, 9, 1, 4};
        cc_partition(r.data(), r.data(), 4, 8, 2, poc, pw);
        CHECK(poc == std::vector<int32_t>({2, 0, -1, 1}), "largest first");
        CHECK(pw == std::vector<int64_t>({9, 4, 2, 0, 0, 0, 0, 0}), "largest first: sums");
        cc_partition(r.data(), r.data(), 4, 2, 1, poc, pw);      // min_reads 1 takes the lone read: 9 | 4 + 2 + 1
        CHECK(poc == std::vector<int32_t>({1, 0, 1, 1}) && pw == std::vector<int64_t>({9, 7}), "min_reads 1");
        cc_partition(r.data(), r.data(), 4, 1, 2, poc, pw);
        CHECK(poc == std::vector<int32_t>({0, 0, -1, 0}) && pw == std::vector<int64_t>({15}), "one part");
    }
    {   // weights that are not the read counts (bases), zero weights and weights past 2^32
        check_one({2, 2, 3, 1, 2}, {0, 0, 0, 7, 0}, 3, 2, "zero weights");
        check_one({2, 3, 2, 5}, {(int64_t)1 << 40, ((int64_t)1 << 40) + 1, (int64_t)1 << 33, 12}, 2, 2, "wide weights");
    }
    std::mt19937_64 rng(12345);
    for (int it = 0; it < 4000; ++it) {
        const int n = (int)(rng() % 60), nparts = 1 + (int)(rng() % (it % 7 == 0 ? 100 : 9));
        const int64_t span = it % 3 == 0 ? 4 : it % 3 == 1 ? 1000 : ((int64_t)1 << 36);      // many ties | few | wide
        std::vector<int64_t> reads((size_t)n), weight((size_t)n);
        for (int c = 0; c < n; ++c) { reads[(size_t)c] = 1 + (int64_t)(rng() % 6); weight[(size_t)c] = it % 2 ? reads[(size_t)c] : (int64_t)(rng() % (uint64_t)span); }
        check_one(reads, weight, nparts, (int64_t)(rng() % 4), "random");
    }
    if (g_failed) { printf("%d of %d checks failed\n", g_failed, g_checks); return 1; }
    printf("ok %d\n", g_checks);
    return 0;
}
