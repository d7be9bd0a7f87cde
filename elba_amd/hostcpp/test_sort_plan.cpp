// test_sort_plan — walks csrc/sort_plan.hpp without the library: the one-word layout of the k-mer stage's sort for every odd k, the memory plan of
// the multi-word sort on both sides of its thresholds, and the cut of the value space into passes on shaped histograms.  Prints one line per failed
// check and "ok <checks>" at the end (tests/test_sort_plan_cpu.py reads it); exit status 1 if a check failed.
#include "../csrc/sort_plan.hpp"
#include <cmath>
#include <cstdio>
#include <functional>
#include <random>

using namespace elba;
typedef std::vector<unsigned long long> Hist;

static int g_checks = 0, g_failed = 0;
#define CHECK(cond, ...) do { ++g_checks; if (!(cond)) { ++g_failed; printf("FAILED %s:%d %s | ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } while (0)

constexpr uint32_t NB = 1u << OWNER_BITS;

static void test_sort_word()
{
    std::vector<uint64_t> Is = {0, 1};
    for (int b = 1; b <= 33; ++b) for (uint64_t I : {(1ull << b) - 1, 1ull << b, (1ull << b) + 1}) Is.push_back(I);
    Is.push_back(1ull << 62); Is.push_back(1ull << 63); Is.push_back(~0ull);      // (the cap of the index bits)
    for (int k = 3; k <= 31; k += 2) for (uint64_t I : Is) for (int kd = 0; kd <= 4; ++kd) for (int pairs = 0; pairs < 2; ++pairs) {
        const SortWord w = plan_sort_word(k, I, kd, pairs != 0);
        int ib = 1;
        while (ib < 63 && (I >> ib) != 0) ++ib;
        CHECK(ib == 63 || (I >> ib) == 0, "I=%llu ib=%d", (unsigned long long)I, ib);
        CHECK(ib == 1 || (I >> (ib - 1)) != 0, "I=%llu ib=%d: not the smallest", (unsigned long long)I, ib);
        int drop = std::max(2 * k + ib - 64, 0);
        if (kd <= 3 && kd < ib && kd > drop) drop = kd;
        CHECK(w.packed_words == (drop <= 3 && !pairs), "k=%d I=%llu kd=%d pairs=%d", k, (unsigned long long)I, kd, pairs);
        if (w.packed_words) {
            CHECK(w.ib == ib && w.drop == drop && w.pb == ib - drop, "k=%d I=%llu kd=%d: ib=%d drop=%d pb=%d", k, (unsigned long long)I, kd, w.ib, w.drop, w.pb);
            CHECK(2 * k + w.pb <= 64 && w.pb >= 1, "k=%d I=%llu kd=%d: pb=%d", k, (unsigned long long)I, kd, w.pb);
            CHECK(ib == 63 || ((I - (I > 0)) >> w.drop) >> w.pb == 0, "k=%d I=%llu: the largest index does not fit pb=%d", k, (unsigned long long)I, w.pb);
        } else CHECK(w.ib == 0 && w.drop == 0 && w.pb == 0, "k=%d I=%llu kd=%d pairs=%d: ib=%d drop=%d pb=%d", k, (unsigned long long)I, kd, pairs, w.ib, w.drop, w.pb);
    }
    // the shapes the tests and the product meet: k = 17 packs up to 2^30 instances whole, drops up to 3 bits up to 2^33; k >= 19 from 2^29 on is pairs
    CHECK(plan_sort_word(17, (1ull << 30) - 1, 0, false).drop == 0 && plan_sort_word(17, 1ull << 30, 0, false).drop == 1, "k=17 at 2^30");
    CHECK(plan_sort_word(17, (1ull << 33) - 1, 0, false).packed_words && !plan_sort_word(17, 1ull << 33, 0, false).packed_words, "k=17 at 2^33");
    CHECK(!plan_sort_word(31, 500000, 0, false).packed_words && plan_sort_word(31, 3, 0, false).packed_words, "k=31");
}

static void test_capacity()
{
    const double out_literal[2][3] = {{45.0, 31.5, 19.8}, {54.0, 36.0, 20.4}};
    const int lowers[3] = {1, 2, 15};
    for (int words = 2; words <= 3; ++words) for (int li = 0; li < 3; ++li) for (uint64_t I : {1000000ull, (1ull << 32) - 17, (1ull << 32) - 16, 5000000000ull}) {
        const int lower = lowers[li];
        const double opb = words == 2 ? 103.5 : 121.5, pb = words == 2 ? 91.0 : 109.0, ob = out_literal[words - 2][li];
        const uint64_t need = std::min<uint64_t>(I, 1ull << 24);
        // the three thresholds of avail: one pass fits; the room holds passes of `need` instances; there is any room at all
        const double t_one = (double)I * (opb + ob), t_fits = ob * (double)I + pb * (double)need, t_room = ob * (double)I;
        for (uint64_t opt_cap : {1ull, 3000ull, (unsigned long long)I, 0xE0000000ull}) for (double t : {t_one, t_fits, t_room}) for (double side : {-1024.0, 1024.0}) {
            const double avail = t + side;
            const LongCapacity c = plan_long_capacity(I, words, lower, avail, opt_cap);
            CHECK(c.one_pass_bytes == opb && c.pass_bytes == pb && std::fabs(c.out_bytes - ob) < 1e-9, "words=%d lower=%d: %.3f %.3f %.3f", words, lower, c.one_pass_bytes, c.pass_bytes, c.out_bytes);
            CHECK(c.one_pass == (I < 0xFFFFFFF0ull && I <= opt_cap && (double)I * (c.one_pass_bytes + c.out_bytes) <= avail), "words=%d I=%llu cap=%llu avail=%.0f", words, (unsigned long long)I, (unsigned long long)opt_cap, avail);
            if (t == t_one && I < 0xFFFFFFF0ull && I <= opt_cap) CHECK(c.one_pass == (side > 0), "words=%d lower=%d I=%llu: one pass at %+.0f", words, lower, (unsigned long long)I, side);
            if (I >= 0xFFFFFFF0ull || I > opt_cap) CHECK(!c.one_pass, "I=%llu cap=%llu", (unsigned long long)I, (unsigned long long)opt_cap);
            CHECK(std::fabs(c.room - (avail - ob * (double)I)) <= 1e-3, "room %.3f", c.room);
            CHECK(c.mem_cap == (c.room > 0 ? (uint64_t)(c.room / c.pass_bytes) : 0), "mem_cap");
            if (t == t_room) CHECK((c.mem_cap == 0) == (side < 0) && c.mem_cap <= 1024, "words=%d I=%llu: mem_cap=%llu at %+.0f", words, (unsigned long long)I, (unsigned long long)c.mem_cap, side);
            CHECK(c.fits == (c.mem_cap >= need), "fits");
            if (t == t_fits) CHECK(c.fits == (side > 0), "words=%d lower=%d I=%llu: fits=%d at %+.0f (mem_cap %llu)", words, lower, (unsigned long long)I, (int)c.fits, side, (unsigned long long)c.mem_cap);
            CHECK(c.cap >= 1 && c.cap <= 0xE0000000ull && c.cap <= std::max<uint64_t>(opt_cap, 1) && c.cap <= std::max<uint64_t>(c.mem_cap, 1), "cap=%llu", (unsigned long long)c.cap);
            CHECK(c.cap == std::max<uint64_t>(std::min<uint64_t>(std::min<uint64_t>(opt_cap, c.mem_cap), 0xE0000000ull), 1), "cap=%llu", (unsigned long long)c.cap);
        }
    }
}

// A histogram over the 24-bit prefixes, held as the 12-bit bins and a rule that spreads a bin over its 4096 prefixes
struct Shape { const char *name; Hist h1; std::function<Hist(uint32_t, unsigned long long)> row; };

static Hist row_even(uint32_t, unsigned long long n) { Hist r(NB, n / NB); for (uint32_t d = 0; d < n % NB; ++d) ++r[d]; return r; }
static Hist row_one_prefix(uint32_t bin, unsigned long long n) { Hist r(NB, 0); r[(bin * 37u + 5u) % NB] = n - n / 8; const Hist rest = row_even(bin, n / 8); for (uint32_t d = 0; d < NB; ++d) r[d] += rest[d]; return r; }
static Hist row_random(uint32_t bin, unsigned long long n)
{
    std::mt19937_64 g(1000 + bin);
    Hist r(NB, 0);
    for (int piece = 0; piece < 16 && n > 0; ++piece) { const unsigned long long x = piece == 15 ? n : g() % (n + 1); r[g() % NB] += x; n -= x; }
    return r;
}

static void check_cut(const Shape &sh, uint64_t cap)
{
    uint64_t I = 0;
    for (unsigned long long x : sh.h1) I += x;
    const HeavyBins hv = heavy_bins(sh.h1, cap);
    CHECK(hv.slot.size() == NB, "%s", sh.name);
    Hist h2;
    size_t nheavy = 0;
    for (uint32_t b = 0; b < NB; ++b) {
        CHECK((hv.slot[b] >= 0) == (sh.h1[b] > cap), "%s cap=%llu bin %u", sh.name, (unsigned long long)cap, b);
        if (hv.slot[b] < 0) continue;
        CHECK((size_t)hv.slot[b] == nheavy && hv.bins[nheavy] == b, "%s cap=%llu bin %u: slot %d", sh.name, (unsigned long long)cap, b, hv.slot[b]);
        const Hist r = sh.row(b, sh.h1[b]);
        unsigned long long sum = 0;
        for (unsigned long long x : r) sum += x;
        CHECK(r.size() == NB && sum == sh.h1[b], "%s: the shape's own row of bin %u", sh.name, b);
        h2.insert(h2.end(), r.begin(), r.end());
        ++nheavy;
    }
    CHECK(hv.bins.size() == nheavy, "%s", sh.name);
    const std::vector<LongPass> passes = cut_long_passes(sh.h1, hv.bins, h2, I, cap);
    CHECK(!passes.empty() && passes.front().lo == 0 && passes.back().hi == 1u << LONG_PREFIX_BITS, "%s cap=%llu: %zu passes", sh.name, (unsigned long long)cap, passes.size());
    // the units in ascending order, walked beside the passes
    uint64_t total = 0;
    size_t q = 0;
    uint64_t sum = 0, nonzero = 0, above = 0, n_above = 0, rest = 0;      // (of the pass; of the input: the units above the cap, what the others hold)
    auto close = [&]() {
        const LongPass &p = passes[q];
        CHECK(p.n == sum, "%s cap=%llu pass %zu [%u, %u): n=%llu, its units hold %llu", sh.name, (unsigned long long)cap, q, p.lo, p.hi, (unsigned long long)p.n, (unsigned long long)sum);
        CHECK(nonzero <= 1 || p.n <= cap, "%s cap=%llu pass %zu: %llu units hold %llu", sh.name, (unsigned long long)cap, q, (unsigned long long)nonzero, (unsigned long long)p.n);
        CHECK(above == 0 || nonzero == 1, "%s cap=%llu pass %zu: a unit above the cap shares its pass", sh.name, (unsigned long long)cap, q);
        CHECK(p.n > 0 || q + 1 == passes.size(), "%s cap=%llu pass %zu of %zu is empty", sh.name, (unsigned long long)cap, q, passes.size());
        total += p.n; sum = 0; nonzero = 0; above = 0;
    };
    auto unit = [&](uint32_t start, unsigned long long x) {
        if (q < passes.size() && start == passes[q].hi) { close(); ++q; }
        if (q >= passes.size()) return;
        CHECK(start >= passes[q].lo && start < passes[q].hi, "%s cap=%llu: unit %u outside pass %zu [%u, %u)", sh.name, (unsigned long long)cap, start, q, passes[q].lo, passes[q].hi);
        sum += x; nonzero += x > 0; above += x > cap;
        if (x > cap) ++n_above; else rest += x;
    };
    for (uint32_t b = 0; b < NB; ++b) {
        if (hv.slot[b] >= 0) for (uint32_t d = 0; d < NB; ++d) unit((b << OWNER_BITS) | d, h2[(size_t)hv.slot[b] * NB + d]);
        else unit(b << OWNER_BITS, sh.h1[b]);
    }
    CHECK(q + 1 == passes.size(), "%s cap=%llu: the units end in pass %zu of %zu", sh.name, (unsigned long long)cap, q, passes.size());
    if (q < passes.size()) close();
    CHECK(total == I, "%s cap=%llu: the passes hold %llu of %llu", sh.name, (unsigned long long)cap, (unsigned long long)total, (unsigned long long)I);
    // a pass without a unit above the cap holds at most the cap: ceil(I / cap) passes at least — and where units above the cap are passes of their
    // own, as many passes as what is left needs, and theirs
    CHECK(passes.size() >= (rest + cap - 1) / cap + n_above, "%s cap=%llu: %zu passes, %llu units above the cap", sh.name, (unsigned long long)cap, passes.size(), (unsigned long long)n_above);
    if (n_above == 0) CHECK(passes.size() >= (I + cap - 1) / cap, "%s cap=%llu: %zu passes", sh.name, (unsigned long long)cap, passes.size());
    for (size_t i = 0; i < passes.size(); ++i) {
        CHECK(passes[i].lo < passes[i].hi && (i == 0 || passes[i].lo == passes[i - 1].hi), "%s cap=%llu pass %zu [%u, %u)", sh.name, (unsigned long long)cap, i, passes[i].lo, passes[i].hi);
        CHECK((passes[i].lo & (NB - 1)) == 0 || hv.slot[passes[i].lo >> OWNER_BITS] >= 0, "%s cap=%llu pass %zu starts at 0x%06x inside a light bin", sh.name, (unsigned long long)cap, i, passes[i].lo);
    }
}

static void test_cuts()
{
    std::vector<Shape> shapes;
    shapes.push_back({"uniform", Hist(NB, 250), row_even});
    { Hist h(NB, 0); h[1234] = 1000000; shapes.push_back({"one bin, spread", h, row_even}); shapes.push_back({"one bin, one prefix", h, row_one_prefix}); }
    { Hist h(NB, 100); h[7] = 600000; shapes.push_back({"a prefix above the cap", h, row_one_prefix}); }
    { Hist h(NB, 100); h[4000] = 800000; h[4001] = 500000; shapes.push_back({"heavy bins over many prefixes", h, row_even}); }
    shapes.push_back({"all zero", Hist(NB, 0), row_even});
    { Hist h(NB, 200); for (uint32_t b = 0; b < 100; ++b) h[b] = h[NB - 1 - b] = 0; shapes.push_back({"zeros at both ends", h, row_random}); }
    for (int seed = 1; seed <= 2; ++seed) {
        std::mt19937_64 g(seed);
        Hist h(NB, 0);
        for (uint32_t b = 0; b < NB; ++b) h[b] = g() % 4 == 0 ? 0 : (g() % 64 == 0 ? g() % 200000 : g() % 500);
        shapes.push_back({"random", h, row_random});
    }
    // (cap 1 makes every bin with instances a heavy one, 16 M units to walk: left to the one-bin shapes, the one with zeros at both ends and the small inputs below)
    for (const Shape &sh : shapes) {
        uint64_t I = 0;
        for (unsigned long long x : sh.h1) I += x;
        for (uint64_t cap : {(uint64_t)(sh.name[0] == 'o' || sh.name[0] == 'z' ? 1 : 257), (uint64_t)257, I / 1000 + 1, I / 50 + 1, I / 7 + 1, I / 3 + 1, I / 2, I / 2 + 1, I - (I > 1), std::max<uint64_t>(I, 1), I + 1, (uint64_t)0xE0000000ull})
            if (cap >= 1) check_cut(sh, cap);
    }
    // few instances, every cap from 1 to I
    for (int seed = 12; seed <= 13; ++seed) {
        std::mt19937_64 g(seed);
        Hist h(NB, 0);
        for (int i = 0; i < 40; ++i) h[seed == 13 ? 9 + g() % 3 : g() % NB] += 1 + g() % 3 / 2;
        const Shape sh{"few", h, row_random};
        uint64_t I = 0;
        for (unsigned long long x : h) I += x;
        for (uint64_t cap = 1; cap <= I; ++cap) check_cut(sh, cap);
    }
}

static void test_check()
{
    const double pass_bytes = 91.0, room = 91.0 * 1e9;
    const LongPass ok{0, 1, 1000}, big{1, 2, 2000000000ull}, huge{2, 3, 0xFFFFFFF0ull}, edge{3, 4, 0xFFFFFFEFull}, fits{4, 5, 1000000000ull};
    LongPassFault f = check_long_passes({ok, fits, ok}, room, pass_bytes);
    CHECK(f.kind == LongPassFault::NONE, "kind %d", (int)f.kind);
    f = check_long_passes({}, room, pass_bytes);
    CHECK(f.kind == LongPassFault::NONE, "no pass: kind %d", (int)f.kind);
    f = check_long_passes({ok, big, huge}, room, pass_bytes);
    CHECK(f.kind == LongPassFault::NO_ROOM && f.index == 1, "kind %d index %zu", (int)f.kind, f.index);
    f = check_long_passes({ok, huge, big}, room, pass_bytes);      // (it does not fit either: the 2^32 test comes first)
    CHECK(f.kind == LongPassFault::TOO_MANY && f.index == 1, "kind %d index %zu", (int)f.kind, f.index);
    f = check_long_passes({ok, huge, big}, 1e18, pass_bytes);
    CHECK(f.kind == LongPassFault::TOO_MANY && f.index == 1, "kind %d index %zu", (int)f.kind, f.index);
    f = check_long_passes({edge}, 1e18, pass_bytes);
    CHECK(f.kind == LongPassFault::NONE, "2^32 - 17 instances are a pass: kind %d", (int)f.kind);
    f = check_long_passes({ok, edge}, room, pass_bytes);
    CHECK(f.kind == LongPassFault::NO_ROOM && f.index == 1, "kind %d index %zu", (int)f.kind, f.index);
    f = check_long_passes({fits}, 91.0 * 1e9 - 1.0, pass_bytes);
    CHECK(f.kind == LongPassFault::NO_ROOM && f.index == 0, "one byte short: kind %d", (int)f.kind);
    f = check_long_passes({ok}, -5.0, pass_bytes);
    CHECK(f.kind == LongPassFault::NO_ROOM && f.index == 0, "no room at all: kind %d", (int)f.kind);
    CHECK(kmer_words(31) == 1 && kmer_words(33) == 2 && kmer_words(63) == 2 && kmer_words(65) == 3 && kmer_words(95) == 3, "kmer_words");
    CHECK(OWNER_BITS == 12 && LONG_PREFIX_BITS == 2 * OWNER_BITS, "a pass boundary is a bin or one of its 4096 prefixes");
}

int main()
{
    test_sort_word();
    test_capacity();
    test_cuts();
    test_check();
    printf("ok %d\n", g_checks - g_failed);
    return g_failed ? 1 : 0;
}
