// msd_plan.hpp — the decisions of the k-mer stage's two-level partition (kmer_msd.hip, msd_run) as pure host arithmetic: which partition an input
// takes (MsdPlan) and how value-range batching cuts it into passes (plan_narrow_passes, plan_wide_passes).  No HIP, no context: plain values in,
// plain values out — hostcpp/test_msd_plan.cpp walks them without a GPU.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>
#include "csr_plan.hpp"      // bits_needed_u; the layout of the CSR sort keys the stage's emit kernels write

namespace elba {

// (16384-key tiles, 139 KB of LDS, one workgroup per CU: on 1024 lanes x 16 keys — sixteen wavefronts to hide the barriers — the partition of
//  config 3 takes 26.4 ms, on 512 x 32 27.6 ms)
constexpr int MT_THREADS = 1024, MT_ITEMS = 16;      // lanes of a workgroup of the partition's kernels, keys per lane
constexpr int W2_THREADS = 512, W2_ITEMS = 16;       // the same for the 16-byte records of 19 <= k <= 31
constexpr int MT_TILE = MT_THREADS * MT_ITEMS;      // instances per tile; a wavefront's share is at most one block of the instance -> read table
constexpr int MT_MAXBITS = 9;
constexpr int VBITS = 16;                     // value bits left to the bucket kernel (two halves of 2^15 values)
constexpr int W2_TILE = W2_THREADS * W2_ITEMS;      // 8192 records of 16 bytes: 128 KB of LDS (runs of 8 records per digit and tile; 4096-record tiles: partition 78 -> 58 ms on 2.0 G instances)
constexpr int W2_MAXBITS = 10;
constexpr uint32_t HINT_MAX_COL = 12;     // longer columns are not examined: a row owns no pair of an L-read column with probability 2^-(L-1), and the test costs L loads
constexpr uint32_t ES_CAP_MAX = 12288;      // entries of a bucket the widest emit kernel sorts in LDS
constexpr uint64_t MSD_PASS_LIMIT = 0xFFFFFFF0ull;      // a pass (or an unbatched input) holds fewer instances: 32-bit places

// the options msd_run's decisions read (Ctx::opt's, by name)
struct MsdOptions { int kmer_msd = 0, msd_wide_bits = 0, msd_rank = 0, msd_no_rank = 0, msd_small_cap = 0; long long kmer_batch_instances = 0; };

// triN < 0: reads (k, lower, upper, nrows = the reads, maxpos = the longest read's last k-mer position: reads_maxpos); triN >= 0: a matrix handed
// over as device triples of triN columns (nrows = its rows, maxpos = its largest position; k, lower, upper are not read)
struct MsdInput { int k = 0; uint64_t I = 0; uint32_t lower = 0, upper = 0; uint64_t maxpos = 0; int64_t nrows = 0, triN = -1; };

inline uint64_t reads_maxpos(uint32_t max_read_len, int k) { return max_read_len >= (uint32_t)k ? max_read_len - (uint32_t)k : 0; }

struct MsdPlan {
    bool ok = false;                  // false: no plan — the input keeps the sort path (every other field is then meaningless)
    bool tri = false, wide = false;   // device triples; 16-byte records (19 <= k <= 31)
    bool batched = false;             // value-range passes
    bool too_many_tiles = false;      // more than 2^45 instances: the caller refuses
    int k = 0, k2 = 0, T = 0, vb = VBITS;      // partitioned bits; value bits below them
    int b1 = 0, b2 = 0, pbits = 0, PB = 0, mb = 0, rk = 0;      // MsdParams' fields (kmer_msd.hip); mb: bits of a row id
    uint32_t rkmask = 0xFFFFFFFFu, dup = 0;
    uint32_t lower = 0, upper = 0;
    uint64_t I = 0, maxpos = 0, batch_cap = 0;
    int64_t nrows = 0;
    uint32_t nb1 = 0, nb2 = 0, nbuckets = 0;      // the whole input's partition (the wide partition's passes choose their own)
    uint32_t tile = 0, ntiles1 = 0, ntiles2 = 0;
    uint32_t nb1_cap = 0, nbk_cap = 0;            // the most first digits / buckets of any pass
    uint32_t small_cap = ES_CAP_MAX;
};

inline MsdPlan plan_msd(const MsdInput &in, const MsdOptions &opt)
{
    MsdPlan p{};
    const bool tri = in.triN >= 0;
    const int k = tri ? 17 : in.k, k2 = 2 * k;
    const uint64_t I = in.I;
    p.tri = tri; p.k = k; p.k2 = k2; p.I = I;
    if (k > 31 || (!tri && in.upper > 255) || I == 0) return p;
    // k <= 17: the partition takes all but 16 value bits.  19 <= k <= 31 ("wide", 16-byte records): as many bits as make a bucket of ~1500 instances
    const bool wide = !tri && k2 - VBITS > 2 * MT_MAXBITS;
    int T = k2 - VBITS, vb = VBITS;
    if (wide) {
        T = 12;
        while (T < 2 * W2_MAXBITS && (I >> T) > 512) ++T;      // (a bucket may hold W2_CAP: six times this average — k-mers are not spread evenly over real genomes)
        if (opt.msd_wide_bits > 0) T = std::min(std::max(opt.msd_wide_bits, 2), 2 * W2_MAXBITS);      // (tests: other splits)
        if (T > k2 - 2) return p;
    }
    if (tri) {
        // buckets of ~2048 entries: 2^vb columns of Z / N entries each; at most 2 x 9 partitioned bits
        if (in.triN < 8) return p;
        const int nbc = bits_needed_u((uint64_t)in.triN - 1);
        const uint64_t avg = (I + (uint64_t)in.triN - 1) / (uint64_t)in.triN;
        vb = 1;
        while (vb < 13 && (avg << (vb + 1)) <= 2048) ++vb;
        if (nbc - vb > 2 * MT_MAXBITS) vb = nbc - 2 * MT_MAXBITS;
        // (a bucket holds at most 1024 columns: the emit kernels keep a column table of half their capacity + 1 — enough for k-mers, which come with LOWER >= 2
        //  entries each, and for 1024 one-entry columns in the smallest class; a bucket beyond the largest class sends the whole matrix to the sort: the
        //  average must stay clear of it)
        if (vb > 10 || (avg << vb) > 6144) return p;
        T = nbc - vb;
    }
    if (T < 2) return p;
    // worth it from ~512 instances per bucket on (the bucket kernels pay a few us per bucket whatever it holds: BASELINE config 2 — 530 per bucket — 6.9 ms
    // here, 7.1 ms through the sort); smaller inputs keep the sort
    if (!opt.kmer_msd && (wide ? I < (1ull << 22) : I < ((uint64_t)512 << T))) return p;
    p.wide = wide; p.T = T; p.vb = vb;
    p.maxpos = in.maxpos; p.nrows = in.nrows;
    p.lower = tri ? 1u : in.lower; p.upper = tri ? 0xFFFFu : in.upper;
    p.b1 = (T + 1) / 2; p.b2 = T - p.b1;
    p.pbits = bits_needed_u(in.maxpos);
    p.mb = bits_needed_u((uint64_t)(in.nrows > 0 ? in.nrows - 1 : 0));
    p.PB = p.mb + p.pbits;
    if ((wide ? VBITS : tri ? T + vb : p.b2 + VBITS) + p.PB > 62) return p;      // (the two top bits of a staged entry carry its hint)
    // an entry's column rank inside its bucket (< 8192: the emit kernels take no more entries) above the 16 value bits, where there is room for it
    // ... and where columns grow long enough for one value to fill a sort range of the emit kernels (UPPER beyond HINT_MAX_COL; the wide path ranks its columns anyway)
    p.rk = (p.PB + VBITS + 13 <= 64 && !opt.msd_no_rank && (wide || tri || p.upper > HINT_MAX_COL || opt.msd_rank)) ? p.PB + VBITS : 0;
    if (tri) { p.rk = p.PB; p.rkmask = (1u << vb) - 1u; p.dup = 1u; }      // (the rank of a column inside its bucket = the low bits of its id: every column holds entries, or the matrix is refused by the driver)
    p.nb1 = 1u << p.b1; p.nb2 = 1u << p.b2; p.nbuckets = p.nb1 * p.nb2;
    p.tile = wide ? (uint32_t)W2_TILE : (uint32_t)MT_TILE;
    // more instances than a 32-bit place holds (or than "kmer_batch_instances": tests): passes over value ranges (reads)
    p.batch_cap = opt.kmer_batch_instances > 0 ? (uint64_t)opt.kmer_batch_instances : 0xE0000000ull;
    p.batched = !tri && I > p.batch_cap;
    if (!p.batched && I >= MSD_PASS_LIMIT) return p;      // (the caller refuses: the sort and the triples hold 32-bit places)
    p.too_many_tiles = (I + p.tile - 1) / p.tile >= MSD_PASS_LIMIT;
    // the bucket arrays hold the most first digits / buckets of any pass: the wide partition's passes choose their own (up to 2^10 x 2^10)
    p.nb1_cap = wide && p.batched ? 1u << W2_MAXBITS : p.nb1;
    p.nbk_cap = wide && p.batched ? (1u << W2_MAXBITS) << W2_MAXBITS : p.nbuckets;
    p.ntiles1 = (uint32_t)((I + p.tile - 1) / p.tile); p.ntiles2 = p.ntiles1 + p.nb1_cap;
    p.small_cap = opt.msd_small_cap > 0 && (uint32_t)opt.msd_small_cap < ES_CAP_MAX ? (uint32_t)opt.msd_small_cap : ES_CAP_MAX;
    p.ok = true;
    return p;
}

// VALUE-RANGE BATCHING: a pass of whole first digits [dlo, dhi) and what phase A learns of it
// (nb1, nb2, T, e: the pass's partition — fixed for k <= 17; the wide partition's passes cut their range finer; N, Z: its k-mers and entries; ncrowded,
//  crowded_small, np: its crowded buckets, those with a small folded entry count, its pseudo-buckets)
struct Pass { uint32_t dlo = 0, dhi = 0; uint64_t I = 0, N = 0, Z = 0; uint32_t nb1 = 0, nb2 = 0; int T = 0, e = 0; int64_t ncrowded = 0, crowded_small = 0; uint32_t np = 0; };

// the input as ONE pass
inline Pass whole_pass(const MsdPlan &p) { Pass w{}; w.dlo = 0; w.dhi = p.nb1; w.I = p.I; w.nb1 = p.nb1; w.nb2 = p.nb2; w.T = p.T; return w; }

// k <= 17: passes of consecutive first digits, each filled up to the cap; a pass takes whole digits — one digit may hold most of the input (a
// homopolymer, AT-rich reads) and is then a pass of its own, larger than the cap.  dt: the instances of every first digit.  *oversized (if given): a
// digit that alone holds MSD_PASS_LIMIT instances or more (the caller refuses), -1: none; planning stops at it.
inline std::vector<Pass> plan_narrow_passes(const std::vector<unsigned long long> &dt, uint64_t batch_cap, uint32_t nb2, int T, int64_t *oversized = nullptr)
{
    const uint32_t nb1 = (uint32_t)dt.size();
    std::vector<Pass> passes;
    if (oversized) *oversized = -1;
    for (uint32_t d = 0; d < nb1;) {
        Pass ps1{}; ps1.dlo = d;
        do { ps1.I += dt[d]; ++d; } while (d < nb1 && ps1.I + dt[d] <= batch_cap);
        ps1.dhi = d; ps1.nb1 = nb1; ps1.nb2 = nb2; ps1.T = T;
        if (ps1.I >= MSD_PASS_LIMIT) { if (oversized) *oversized = (int64_t)ps1.dlo; return passes; }
        if (ps1.I) passes.push_back(ps1);
    }
    return passes;
}

// 19 <= k <= 31: planned on the coarse digit (the leading W2_MAXBITS bits of the flattened value); passes of whole coarse digits, balanced (as many
// as the cap demands, each near I / passes: the partition buffers are sized by the largest).  A pass partitions its own range: its first level takes
// e more bits of each of its coarse digits ((dhi - dlo) << e <= 2^10 digits), its second level b2 <= 10 bits, chosen as T is for one pass — a pass's
// buckets are as fine as those of an input of its size ("msd_wide_bits": the pass's T = 10 + e + b2 instead, b2 >= 1).
inline std::vector<Pass> plan_wide_passes(const std::vector<unsigned long long> &dt, uint64_t I, uint64_t batch_cap, int msd_wide_bits, int64_t *oversized = nullptr)
{
    const uint32_t nd = (uint32_t)dt.size();      // (W2_MAXBINS)
    std::vector<Pass> passes;
    if (oversized) *oversized = -1;
    const uint64_t npass = (I + batch_cap - 1) / batch_cap, target = (I + npass - 1) / npass;
    for (uint32_t d = 0; d < nd;) {
        Pass p1{}; p1.dlo = d;
        do { p1.I += dt[d]; ++d; } while (d < nd && p1.I + dt[d] <= batch_cap && p1.I + dt[d] / 2 <= target);
        p1.dhi = d;
        if (p1.I >= MSD_PASS_LIMIT) { if (oversized) *oversized = (int64_t)p1.dlo; return passes; }
        if (!p1.I) continue;
        int e1 = 0;
        while (e1 < W2_MAXBITS && ((p1.dhi - p1.dlo) << (e1 + 1)) <= nd) ++e1;
        p1.e = e1; p1.nb1 = (p1.dhi - p1.dlo) << e1;
        int b2 = 1;
        while (b2 < W2_MAXBITS && ((p1.I >> b2) / p1.nb1) > 512) ++b2;
        if (msd_wide_bits > 0) b2 = std::min(std::max(msd_wide_bits - W2_MAXBITS - e1, 1), W2_MAXBITS);
        p1.nb2 = 1u << b2; p1.T = W2_MAXBITS + e1 + b2;
        passes.push_back(p1);
    }
    return passes;
}

}  // namespace elba
