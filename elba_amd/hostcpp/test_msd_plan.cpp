// test_msd_plan — walks csrc/msd_plan.hpp without the library: the plan of the two-level k-mer partition for every odd k, and the two planners of
// value-range batching on shaped digit totals.  Prints one line per failed check and "ok <checks>" at the end (tests/test_msd_plan_cpu.py reads it);
// exit status 1 if a check failed.
#include "../csrc/msd_plan.hpp"
#include <cstdio>
#include <string>

using namespace elba;
typedef std::vector<unsigned long long> Totals;

static int g_checks = 0, g_failed = 0;
#define CHECK(cond, ...) do { ++g_checks; if (!(cond)) { ++g_failed; printf("FAILED %s:%d %s | ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } while (0)

static MsdInput reads_in(int k, uint64_t I, uint32_t upper = 8) { MsdInput in{}; in.k = k; in.I = I; in.lower = 2; in.upper = upper; in.maxpos = reads_maxpos(20000, k); in.nrows = 100000; return in; }
static MsdInput triples_in(uint64_t Z, int64_t N) { MsdInput in{}; in.I = Z; in.maxpos = 20000; in.nrows = 100000; in.triN = N; return in; }

static void test_plans()
{
    MsdOptions forced{}; forced.kmer_msd = 1;
    for (int k = 9; k <= 31; k += 2) for (uint64_t I : {1000ull, 1ull << 22, 3ull << 30}) {
        const MsdPlan p = plan_msd(reads_in(k, I), forced);
        CHECK(p.ok, "k=%d I=%llu", k, (unsigned long long)I);
        CHECK(p.wide == (k >= 19) && !p.tri && !p.batched, "k=%d", k);
        if (!p.wide) CHECK(p.b1 + p.b2 + VBITS == 2 * k && p.T == 2 * k - VBITS, "k=%d b1=%d b2=%d", k, p.b1, p.b2);
        else CHECK(p.T >= 12 && p.T <= 20 && p.T <= 2 * k - 2, "k=%d T=%d", k, p.T);
        CHECK(p.b1 == (p.T + 1) / 2 && p.b1 + p.b2 == p.T, "k=%d T=%d b1=%d", k, p.T, p.b1);
        CHECK(p.nb1 == 1u << p.b1 && p.nb2 == 1u << p.b2 && p.nbuckets == p.nb1 * p.nb2 && p.nb1_cap == p.nb1 && p.nbk_cap == p.nbuckets, "k=%d", k);
        CHECK(p.tile == (uint32_t)(p.wide ? W2_TILE : MT_TILE) && p.ntiles1 == (I + p.tile - 1) / p.tile && p.ntiles2 == p.ntiles1 + p.nb1_cap, "k=%d", k);
        CHECK(p.PB == p.mb + p.pbits && p.mb == 17 && p.pbits == bits_needed_u(reads_maxpos(20000, k)), "k=%d PB=%d", k, p.PB);
        CHECK(p.small_cap == ES_CAP_MAX, "k=%d", k);
        // the column rank: above the value bits or nowhere; never past bit 64 with its 13 bits
        for (int rank = 0; rank < 2; ++rank) for (int no_rank = 0; no_rank < 2; ++no_rank) for (uint32_t upper : {8u, 40u, 255u}) for (uint64_t maxpos : {200ull, 20000ull, (1ull << 22) - 1, (1ull << 28) - 1}) {
            MsdOptions o = forced; o.msd_rank = rank; o.msd_no_rank = no_rank;
            MsdInput in = reads_in(k, I, upper); in.maxpos = maxpos;
            const MsdPlan q = plan_msd(in, o);
            if (!q.ok) { CHECK((q.wide ? VBITS : q.b2 + VBITS) + q.PB > 62, "k=%d maxpos=%llu: no plan", k, (unsigned long long)maxpos); continue; }
            CHECK(q.rk == 0 || q.rk == q.PB + VBITS, "k=%d rk=%d", k, q.rk);
            CHECK(q.rk + 13 <= 64, "k=%d rk=%d", k, q.rk);
            if (no_rank) CHECK(q.rk == 0, "k=%d: msd_no_rank wins over msd_rank=%d", k, rank);
            else if (q.PB + VBITS + 13 <= 64) CHECK((q.rk != 0) == (q.wide || upper > HINT_MAX_COL || rank), "k=%d upper=%u rank=%d rk=%d", k, upper, rank, q.rk);
            CHECK(q.rkmask == 0xFFFFFFFFu && q.dup == 0u, "k=%d", k);
        }
        CHECK(!plan_msd(reads_in(k, 0), forced).ok, "k=%d: I = 0", k);
        CHECK(!plan_msd(reads_in(k, I, 256), forced).ok, "k=%d: upper > 255", k);
    }
    for (int k : {33, 35, 63}) CHECK(!plan_msd(reads_in(k, 1 << 22), forced).ok, "k=%d > 31", k);
    // unforced: worth it from ~512 instances per bucket (k <= 17) / 2^22 instances (wide) on
    CHECK(!plan_msd(reads_in(17, (512ull << 18) - 1), MsdOptions{}).ok && plan_msd(reads_in(17, 512ull << 18), MsdOptions{}).ok, "k=17 threshold");
    CHECK(!plan_msd(reads_in(31, (1ull << 22) - 1), MsdOptions{}).ok && plan_msd(reads_in(31, 1ull << 22), MsdOptions{}).ok, "k=31 threshold");
    // "msd_wide_bits" clamps T to [2, 20]; "msd_small_cap" below ES_CAP_MAX only
    for (int bits : {1, 2, 11, 16, 30}) { MsdOptions o = forced; o.msd_wide_bits = bits; const MsdPlan p = plan_msd(reads_in(31, 1 << 22), o); CHECK(p.ok && p.T == std::min(std::max(bits, 2), 20), "bits=%d T=%d", bits, p.T); }
    { MsdOptions o = forced; o.msd_wide_bits = 30; CHECK(!plan_msd(reads_in(9, 1000), o).wide, "k=9 is never wide"); }
    { MsdOptions o = forced; o.msd_small_cap = 64; CHECK(plan_msd(reads_in(17, 1000), o).small_cap == 64u, "small_cap 64"); o.msd_small_cap = 20000; CHECK(plan_msd(reads_in(17, 1000), o).small_cap == ES_CAP_MAX, "small_cap 20000"); }
    // value-range batching: beyond the cap; unbatched inputs stay below 32-bit places
    { MsdOptions o = forced; o.kmer_batch_instances = 999; const MsdPlan p = plan_msd(reads_in(17, 1000), o); CHECK(p.ok && p.batched && p.batch_cap == 999 && p.nb1_cap == p.nb1, "k=17 batched");
      const MsdPlan w = plan_msd(reads_in(31, 1000), o); CHECK(w.ok && w.batched && w.nb1_cap == 1024u && w.nbk_cap == 1u << 20 && w.ntiles2 == w.ntiles1 + 1024u, "k=31 batched");
      o.kmer_batch_instances = 1000; CHECK(!plan_msd(reads_in(17, 1000), o).batched, "at the cap: one pass"); }
    { const MsdPlan p = plan_msd(reads_in(17, 0xE0000001ull), forced); CHECK(p.ok && p.batched && p.batch_cap == 0xE0000000ull, "default cap");
      MsdOptions o = forced; o.kmer_batch_instances = 1ll << 40; CHECK(!plan_msd(reads_in(17, MSD_PASS_LIMIT), o).ok && plan_msd(reads_in(17, MSD_PASS_LIMIT - 1), o).ok, "one pass of 2^32 - 16 instances"); }
    // triples
    { const MsdPlan p = plan_msd(triples_in(255325, 60041), forced); CHECK(p.ok && p.tri && !p.wide && !p.batched && p.k == 17 && p.lower == 1u && p.upper == 0xFFFFu, "triples");
      CHECK(p.T + p.vb == bits_needed_u(60040) && p.T <= 2 * MT_MAXBITS && p.vb <= 10 && p.rk == p.PB && p.rkmask == (1u << p.vb) - 1u && p.dup == 1u, "triples T=%d vb=%d", p.T, p.vb); }
    CHECK(!plan_msd(triples_in(7700, 7), forced).ok && plan_msd(triples_in(8800, 8), forced).ok, "triples: N < 8");
    CHECK(!plan_msd(triples_in(1ull << 31, 1ll << 30), forced).ok, "triples: vb > 10 (2^30 columns on 18 partitioned bits)");
    CHECK(!plan_msd(triples_in(3073ull * 16, 16), forced).ok && plan_msd(triples_in(3072ull * 16, 16), forced).ok, "triples: avg << vb > 6144 (vb = 1)");
}

// the passes cover [0, nd) without gap or overlap, in order (empty stretches belong to no pass), and their instances sum to the total
static void check_cover(const std::vector<Pass> &ps, const Totals &dt, const char *what)
{
    uint64_t total = 0, sum = 0;
    for (unsigned long long v : dt) total += v;
    uint32_t at = 0;
    for (const Pass &p : ps) {
        CHECK(p.dlo >= at && p.dlo < p.dhi && p.dhi <= dt.size() && p.I > 0, "%s: pass [%u, %u) after %u", what, p.dlo, p.dhi, at);
        for (uint32_t d = at; d < p.dlo; ++d) CHECK(dt[d] == 0, "%s: digit %u skipped with %llu instances", what, d, dt[d]);
        uint64_t I = 0;
        for (uint32_t d = p.dlo; d < p.dhi && d < dt.size(); ++d) I += dt[d];
        CHECK(I == p.I, "%s: pass [%u, %u) holds %llu, says %llu", what, p.dlo, p.dhi, (unsigned long long)I, (unsigned long long)p.I);
        sum += p.I; at = p.dhi;
    }
    for (uint32_t d = at; d < dt.size(); ++d) CHECK(dt[d] == 0, "%s: digit %u behind the last pass", what, d);
    CHECK(sum == total, "%s: %llu of %llu instances", what, (unsigned long long)sum, (unsigned long long)total);
}

static std::vector<std::pair<std::string, Totals>> shapes(uint32_t nd, unsigned long long each, unsigned long long big)
{
    std::vector<std::pair<std::string, Totals>> out;
    out.push_back({"equal", Totals(nd, each)});
    for (uint32_t at : {0u, nd / 2, nd - 1}) { Totals t(nd, 0); t[at] = big; out.push_back({"one digit at " + std::to_string(at), t}); }
    { Totals t(nd, each); t[nd / 3] = big; out.push_back({"a dominant digit among equal ones", t}); }
    { Totals t(nd, each); t[0] = 0; if (nd > 4) t[1] = 0; out.push_back({"zeros at the front", t}); }
    { Totals t(nd, each); t[nd / 2] = 0; t[nd / 2 - 1] = 0; out.push_back({"zeros in the middle", t}); }
    { Totals t(nd, each); t[nd - 1] = 0; if (nd > 4) t[nd - 2] = 0; out.push_back({"zeros at the end", t}); }
    { Totals t(nd, 0); for (uint32_t d = 0; d < nd; ++d) t[d] = (d * 2654435761u >> 7) % (2 * each + 1); out.push_back({"scattered", t}); }
    return out;
}

static void test_narrow_planner()
{
    for (uint32_t nd : {4u, 16u, 512u}) for (unsigned long long cap : {1000ull, 3500ull, 1ull << 30}) for (const auto &sh : shapes(nd, 1000, MSD_PASS_LIMIT - 1)) {
        const std::string what = "narrow " + std::to_string(nd) + " digits, cap " + std::to_string(cap) + ", " + sh.first;
        int64_t over = 0;
        const std::vector<Pass> ps = plan_narrow_passes(sh.second, cap, 128, 18, &over);
        CHECK(over == -1, "%s: digit %lld reported", what.c_str(), (long long)over);
        check_cover(ps, sh.second, what.c_str());
        for (size_t i = 0; i < ps.size(); ++i) {
            const Pass &p = ps[i];
            CHECK(p.nb1 == nd && p.nb2 == 128u && p.T == 18 && p.e == 0, "%s", what.c_str());
            // over the cap: only a pass whose first digit alone is — and then nothing was added to it
            if (p.I > cap) CHECK(sh.second[p.dlo] > cap && p.I == sh.second[p.dlo], "%s: pass [%u, %u) of %llu", what.c_str(), p.dlo, p.dhi, (unsigned long long)p.I);
            // greedy: the next digit did not fit
            if (p.dhi < nd) CHECK(p.I + sh.second[p.dhi] > cap, "%s: pass [%u, %u) closed early", what.c_str(), p.dlo, p.dhi);
        }
    }
    for (uint32_t nd : {4u, 16u, 512u}) {
        Totals t(nd, 10); t[nd / 2] = MSD_PASS_LIMIT;
        int64_t over = -1;
        plan_narrow_passes(t, 1000, 128, 18, &over);
        CHECK(over == (int64_t)(nd / 2), "narrow %u digits: a digit of 2^32 - 16 instances, reported %lld", nd, (long long)over);
    }
}

static void test_wide_planner()
{
    const uint32_t nd = 1u << W2_MAXBITS;
    for (int bits : {0, 11, 16, 30}) for (unsigned long long cap : {1000ull, 40000ull, 1ull << 30}) for (const auto &sh : shapes(nd, 1000, MSD_PASS_LIMIT - 1)) {
        const std::string what = "wide, cap " + std::to_string(cap) + ", msd_wide_bits " + std::to_string(bits) + ", " + sh.first;
        uint64_t I = 0;
        for (unsigned long long v : sh.second) I += v;
        int64_t over = 0;
        const std::vector<Pass> ps = plan_wide_passes(sh.second, I, cap, bits, &over);
        CHECK(over == -1, "%s: digit %lld reported", what.c_str(), (long long)over);
        check_cover(ps, sh.second, what.c_str());
        const uint64_t npass = (I + cap - 1) / cap, target = (I + npass - 1) / npass;
        for (const Pass &p : ps) {
            const uint32_t span = p.dhi - p.dlo;
            CHECK((span << p.e) <= nd && (p.e == W2_MAXBITS || (span << (p.e + 1)) > nd), "%s: e=%d not maximal for %u digits", what.c_str(), p.e, span);
            CHECK(p.nb1 == span << p.e, "%s", what.c_str());
            int b2 = 0;
            while ((1u << b2) < p.nb2) ++b2;
            CHECK(p.nb2 == 1u << b2 && b2 >= 1 && b2 <= W2_MAXBITS && p.T == W2_MAXBITS + p.e + b2, "%s: nb2=%u T=%d e=%d", what.c_str(), p.nb2, p.T, p.e);
            if (bits > 0) CHECK(b2 == std::min(std::max(bits - W2_MAXBITS - p.e, 1), (int)W2_MAXBITS), "%s: b2=%d e=%d", what.c_str(), b2, p.e);
            else CHECK((b2 == W2_MAXBITS || ((p.I >> b2) / p.nb1) <= 512) && (b2 == 1 || ((p.I >> (b2 - 1)) / p.nb1) > 512), "%s: b2=%d", what.c_str(), b2);
            if (p.I > cap) CHECK(span == 1 || sh.second[p.dlo] == p.I, "%s: pass [%u, %u) of %llu", what.c_str(), p.dlo, p.dhi, (unsigned long long)p.I);
            // closed by the balancing rule or by the cap — or by the end of the digits
            if (p.dhi < nd) CHECK(p.I + sh.second[p.dhi] > cap || p.I + sh.second[p.dhi] / 2 > target, "%s: pass [%u, %u) closed early", what.c_str(), p.dlo, p.dhi);
            // ... and not too late: every digit but its first was added under both rules
            for (uint64_t run = sh.second[p.dlo], d = p.dlo + 1; d < p.dhi; ++d) { CHECK(run + sh.second[d] <= cap && run + sh.second[d] / 2 <= target, "%s: digit %llu joined pass [%u, %u)", what.c_str(), (unsigned long long)d, p.dlo, p.dhi); run += sh.second[d]; }
        }
    }
    Totals t(nd, 10); t[700] = MSD_PASS_LIMIT;
    int64_t over = -1;
    plan_wide_passes(t, MSD_PASS_LIMIT + 10ull * (nd - 1), 1000, 0, &over);
    CHECK(over == 700, "wide: a coarse digit of 2^32 - 16 instances, reported %lld", (long long)over);
}

int main()
{
    test_plans();
    test_narrow_planner();
    test_wide_planner();
    if (g_failed) { printf("failed %d of %d\n", g_failed, g_checks); return 1; }
    printf("ok %d\n", g_checks);
    return 0;
}
