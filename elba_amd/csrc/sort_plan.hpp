// sort_plan.hpp — the decisions of the k-mer stage's SORT path (kmer.hip) as pure host arithmetic: the layout of the one word a k <= 31 instance
// travels in (plan_sort_word), and for the multi-word sort of k > 31 what the memory allows (plan_long_capacity), how the value space is cut into
// passes (heavy_bins, cut_long_passes) and which pass cannot run (check_long_passes).  No HIP, no context: plain values in, plain values out —
// hostcpp/test_sort_plan.cpp walks them without a GPU.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>
#include "msd_plan.hpp"      // MSD_PASS_LIMIT: the 32-bit places every pass of the stage holds

namespace elba {

inline int kmer_words(int k) { return k > 64 ? 3 : (k > 32 ? 2 : 1); }      // (k is odd: 31 is the last one-word k, 63 the last two-word k)
constexpr int OWNER_BITS = 12;            // the value space in 2^12 bins by the leading bits of the first word: the owners' ranges, the passes' coarse units
constexpr int LONG_PREFIX_BITS = 24;      // a pass of the multi-word sort is a range of the leading 24 bits of the first word

// One 64-bit word per instance: value << pb | (instance index >> drop).  The index is the payload — (read, pos) follow from it through the instance
// offsets, for the entries that survive the count filter only — and when value and index are a few bits too many for one word (k = 17 beyond 2^30
// instances) its `drop` lowest bits are left out: the candidates they stand for are told apart afterwards by recomputing their k-mers
// (k_instance_entries).  The sort then moves 8 bytes per instance, not 16.  More than 3 dropped bits, or option kmer_pairs: (value, payload) pairs,
// ib = drop = pb = 0.  kmer_drop: a test hook, small inputs through the dropped-index-bit path.
struct SortWord { int ib = 0, drop = 0, pb = 0; bool packed_words = false; };
inline SortWord plan_sort_word(int k, uint64_t I, int kmer_drop, bool kmer_pairs)
{
    SortWord w;
    w.ib = 1;
    while (w.ib < 63 && (I >> w.ib)) ++w.ib;
    w.drop = 2 * k + w.ib > 64 ? 2 * k + w.ib - 64 : 0;
    if (kmer_drop > w.drop && kmer_drop <= 3 && kmer_drop < w.ib) w.drop = kmer_drop;
    w.packed_words = w.drop <= 3 && !kmer_pairs;
    if (!w.packed_words) { w.ib = 0; w.drop = 0; }
    w.pb = w.ib - w.drop;                  // payload bits below the value
    return w;
}

// Device bytes per instance of the multi-word sort, DevBuf's 1/8 slack included.  One pass (sort_long_one_pass' reservations): khi klo val i0 i1 t0
// t1, ws_a ws_b ws_c (8 each), ws_e (4), ws_f (8); three words: klo2 and s2buf (8 each).  A value-range pass: the same without ws_e / ws_f, which
// the sort path does not use at the instance count, plus the sort's histograms and the wavefront counts (under 1).  The columns: at most I entries
// (a_csc and kid_of_entry, 8 each) and I / LOWER k-mers (the words, count and pointer).
// avail_bytes: what the call may use.  One pass takes the input when it holds fewer than 2^32 instances, no more than opt_cap (option
// kmer_batch_instances, else 0xE0000000) and its workspace and columns fit; otherwise passes of at most `cap` instances, in the `room` the columns
// leave.  fits: the room holds passes of min(I, 2^24) instances (the caller refuses otherwise).
struct LongCapacity { bool one_pass = false, fits = false; uint64_t cap = 1, mem_cap = 0; double room = 0, one_pass_bytes = 0, pass_bytes = 0, out_bytes = 0; };
inline LongCapacity plan_long_capacity(uint64_t I, int words, int lower, double avail_bytes, uint64_t opt_cap)
{
    LongCapacity c;
    c.one_pass_bytes = (words == 2 ? 92.0 : 108.0) * 1.125;
    c.pass_bytes = (words == 2 ? 80.0 : 96.0) * 1.125 + 1.0;
    c.out_bytes = (16.0 + (8.0 * words + 8.0) / (double)std::max(lower, 1)) * 1.125;
    c.one_pass = I < MSD_PASS_LIMIT && I <= opt_cap && (double)I * (c.one_pass_bytes + c.out_bytes) <= avail_bytes;
    c.room = avail_bytes - c.out_bytes * (double)I;                      // for the workspace of the largest pass
    c.mem_cap = c.room > 0 ? (uint64_t)(c.room / c.pass_bytes) : 0;
    c.fits = c.mem_cap >= std::min<uint64_t>(I, 1ull << 24);
    c.cap = std::max<uint64_t>(std::min<uint64_t>(std::min(opt_cap, c.mem_cap), 0xE0000000ull), 1);
    return c;
}

// the 12-bit bins that hold more than the cap, ascending, and slot[bin] = the bin's row of the refining histogram over its 24-bit prefixes, or -1
struct HeavyBins { std::vector<uint32_t> bins; std::vector<int32_t> slot; };
inline HeavyBins heavy_bins(const std::vector<unsigned long long> &h1, uint64_t cap)
{
    HeavyBins h;
    h.slot.assign(h1.size(), -1);
    for (uint32_t b = 0; b < (uint32_t)h1.size(); ++b) if (h1[b] > cap) { h.slot[b] = (int32_t)h.bins.size(); h.bins.push_back(b); }
    return h;
}

// A pass: the range [lo, hi) of 24-bit prefixes and its n instances.  Units in ascending order (a 12-bit bin of h1, or one 24-bit prefix of a heavy
// bin: row `slot` of h2); passes of whole units, balanced as the wide partition's (plan_wide_passes): as many as the cap needs, each near
// I / passes.  A unit above the cap is a pass of its own.
struct LongPass { uint32_t lo, hi; uint64_t n; };
inline std::vector<LongPass> cut_long_passes(const std::vector<unsigned long long> &h1, const std::vector<uint32_t> &heavy, const std::vector<unsigned long long> &h2, uint64_t I, uint64_t cap)
{
    constexpr uint32_t NB = 1u << OWNER_BITS;
    std::vector<LongPass> passes;
    const uint64_t npass = (I + cap - 1) / cap, target = npass ? (I + npass - 1) / npass : 0;
    uint32_t lo = 0;
    uint64_t cnt = 0;
    size_t hv = 0;
    auto unit = [&](uint32_t start, uint64_t x) {
        if (cnt > 0 && (cnt + x > cap || cnt + x / 2 > target)) { passes.push_back(LongPass{lo, start, cnt}); lo = start; cnt = 0; }
        cnt += x;
    };
    for (uint32_t b = 0; b < NB; ++b) {
        if (hv < heavy.size() && heavy[hv] == b) { for (uint32_t d = 0; d < NB; ++d) unit((b << OWNER_BITS) | d, h2[hv * NB + d]); ++hv; }
        else unit(b << OWNER_BITS, h1[b]);
    }
    passes.push_back(LongPass{lo, 1u << LONG_PREFIX_BITS, cnt});
    return passes;
}

// the first pass that cannot run: it holds 2^32 instances or more (TOO_MANY), or its workspace does not fit the room (NO_ROOM)
struct LongPassFault { enum Kind { NONE, TOO_MANY, NO_ROOM } kind = NONE; size_t index = 0; };
inline LongPassFault check_long_passes(const std::vector<LongPass> &passes, double room, double pass_bytes)
{
    for (size_t q = 0; q < passes.size(); ++q) {
        if (passes[q].n >= MSD_PASS_LIMIT) return LongPassFault{LongPassFault::TOO_MANY, q};
        if (!(pass_bytes * (double)passes[q].n <= room)) return LongPassFault{LongPassFault::NO_ROOM, q};
    }
    return LongPassFault{};
}

}  // namespace elba
