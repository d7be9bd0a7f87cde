// ov_plan.hpp — the decisions of the overlap SpGEMM's host driver (spgemm.hip) as pure host arithmetic: which kernel family runs a call and with
// which switches (OvPlan), the ONE table of tier geometry (OV_ROWS), what a repeated pass changes (ov_next_pass) and what a finished call leaves
// as hints (ov_next_hints).  No HIP, no context: plain values in, plain values out — hostcpp/test_ov_plan.cpp walks them without a GPU.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include "csr_plan.hpp"      // the format of a row entry of A (csr_pos_mask)

namespace elba {

constexpr int NUM_LDS_TIERS = 5;                // 512, 1024, 2048, 4096, 8192 slots (18 B per slot incl. the 16-bit survivor list)
constexpr int NUM_TIERS = NUM_LDS_TIERS + 1;    // + HBM spill
constexpr int LDS_TBITS0 = 9;
constexpr uint32_t STAGE_CHUNK = 1024;          // staging entries a workgroup draws from the global cursor at a time
constexpr uint32_t STAGE_REC_BYTES = 32;        // sizeof(StageRec)
constexpr uint32_t FIN_WAVE2_MAX = 1024;        // widest row the one-wave bucket sort takes (wider rows: one workgroup each)
constexpr uint32_t SLAB_PAD = 16;
constexpr int RP_TILE = 1024;                   // row counts a workgroup of k_row_pointers scans
constexpr int FIN_HUGE_BLOCKS = 32;             // workgroups of k_finalize_huge, each with a sort area of its own
constexpr int OV_SAMPLE_ROWS = 256, OV_SAMPLE_TIER = 3;
constexpr size_t OV_LDS_MAX = 160 * 1024;

// what the reads-path instantiation of the numeric kernel fixes at compile time (OvSpecParams takes them from here)
namespace ov_spec {
constexpr uint32_t half = 1, inl = 1, pay16 = 1, rec16 = 1, suffix = 0, qblk_log2 = 0, j_shift = 0;
constexpr uint32_t hint_mask = 1u << 31, pos_mask = csr_pos_mask(false, true);
// ... and what its compiled-geometry variant fixes on top: columns padded to ONE 64-byte line (8 entries: every matrix whose longest column holds 5 .. 8
// entries, matrix.hip: choose_column_store), four lanes x 16 bytes per row entry, 3 bits of a sequence number for the place in the column
constexpr uint32_t geom_stride = 8, geom_lpc_log2 = 2, geom_fbits = 3;
}

// ---- the tier table: one row per (family, tier) — THE place where tier geometry is stated ------------------------------------------------
// block: lanes of a workgroup; tbits: log2 of the table's slots; tbc: the table bits as a template argument (dense rows that compile them in, 0:
// a kernel argument); cu_factor: workgroups per CU (OV_GRID_DENSE_WGS: option "dense_wgs", OV_GRID_SPILL: OvPlan::spill_blocks); slot_bytes: LDS per
// table slot; global / payload / dense: the template arguments G, P and DENSE of k_spgemm_direct.  Behind the table an LDS row keeps 256 bytes of
// misc words and per wavefront one product ring and one row-entry FIFO (ov_row_lds).
enum OvFamily { OV_DENSE, OV_PAY, OV_S32, OV_SHARED };      // dense path (64-bit payload, suffix rows) | 64-bit payload | 32-bit accumulators | both of the latter two
constexpr int OV_GRID_DENSE_WGS = 0, OV_GRID_SPILL = -1;
struct OvTierRow { OvFamily family; int tier, block, tbits, tbc, cu_factor, slot_bytes; bool global, payload, dense; int dense_up_min; };
constexpr OvTierRow OV_ROWS[] = {
    // dense: four wavefronts share a 512-slot table (32 per CU); with "dense_up" >= 1 / 2 tiers 1 / 2 take twice the lanes and compile their table bits in
    {OV_DENSE, 0, 256, 9, 9, OV_GRID_DENSE_WGS, 18, false, false, true, 0},
    {OV_DENSE, 1, 256, 10, 0, 4, 18, false, false, true, 0},
    {OV_DENSE, 1, 512, 10, 10, 4, 18, false, false, true, 1},
    {OV_DENSE, 2, 512, 11, 0, 2, 18, false, false, true, 0},
    {OV_DENSE, 2, 1024, 11, 11, 2, 18, false, false, true, 2},
    {OV_DENSE, 3, 1024, 12, 0, 1, 18, false, false, true, 0},
    // 64-bit accumulators that carry both positions: 26 bytes per slot
    {OV_PAY, 0, 128, 9, 0, 9, 26, false, true, false, 0},
    {OV_PAY, 1, 256, 10, 0, 4, 26, false, true, false, 0},
    {OV_PAY, 2, 512, 11, 0, 2, 26, false, true, false, 0},
    {OV_PAY, 3, 1024, 12, 0, 1, 26, false, true, false, 0},
    // 32-bit accumulators (look-ups, or posT carried: pay16): 18 bytes per slot
    {OV_S32, 0, 128, 9, 0, 12, 18, false, false, false, 0},
    {OV_S32, 1, 256, 10, 0, 7, 18, false, false, false, 0},
    {OV_S32, 2, 512, 11, 0, 3, 18, false, false, false, 0},
    {OV_S32, 3, 1024, 12, 0, 1, 18, false, false, false, 0},
    // every family: 8192 slots under 4 wavefronts (with their rings they fill the 160 KB), and the HBM tier (tables of gstride slots per workgroup)
    {OV_SHARED, 4, 256, 13, 0, 1, 18, false, false, false, 0},
    {OV_SHARED, NUM_LDS_TIERS, 256, 0, 0, OV_GRID_SPILL, 0, true, false, false, 0},
};
constexpr int OV_NROWS = (int)(sizeof(OV_ROWS) / sizeof(OV_ROWS[0]));

// the claimed slots at which a row abandons an LDS tier of 2^tbits slots under `block` lanes: min(3T/4, T - block) - 1 (a lane overshoots by at most one
// claim: Table::insert_lds).  The plan states it per tier (OvPlan::tier_limit); the numeric kernels that compile their table size in take it from here
constexpr uint32_t ov_tier_limit(int tbits, int block) { return std::min(((1u << tbits) >> 2) * 3, (1u << tbits) - (uint32_t)block) - 1; }

// staging records beyond what the rows need: one open chunk per resident workgroup
constexpr int64_t ov_stage_slack(int num_cus) { return (int64_t)num_cus * 32 * STAGE_CHUNK + 64; }

// LDS bytes of a row's launch.  Dense rows: 2368 bytes of rings per wavefront; the others 3072 with the payload, 2048 with pay16, else 2560; the HBM
// tier never packs its FIFO entries (2560)
constexpr size_t ov_row_lds(const OvTierRow &r, bool pay16)
{
    const size_t waves = (size_t)(r.block / 64), table = r.global ? 0 : (size_t)r.slot_bytes << r.tbits;
    return table + 256 + waves * (r.dense ? 2368 : r.global ? 2560 : r.payload ? 3072 : pay16 ? 2048 : 2560);
}

// the row that runs tier `tier` for a family ("dense_up" picks between the dense family's two rows of tiers 1 and 2)
inline int ov_row_of(OvFamily family, int tier, int dense_up)
{
    int found = -1;
    for (int r = 0; r < OV_NROWS; ++r) {
        const OvTierRow &x = OV_ROWS[r];
        if (x.tier == tier && (x.family == family || x.family == OV_SHARED) && dense_up >= x.dense_up_min) found = r;      // (the last row that qualifies: rows of a tier ascend in dense_up_min)
    }
    return found;
}

// ---- input ------------------------------------------------------------------------------------------------------------------------------
// the options the driver's decisions read (Ctx::opt's, by name)
struct OvOptions {
    bool no_symmetry = false, no_pay = false, mir32 = false, no_slab = false, no_sample = false, ov_generic = false;
    bool spec_rt_geom = false;      // option "ov_generic" = 2 (A/B): the reads path keeps its run-time geometry
    int dk = -1, dense_up = 1, dense_wgs = 8, slab_q16 = 0, slab_pct = 175;
    int64_t tune3 = 0, tune4 = 0, tune5 = 0, tune7 = 0;
};
// what earlier calls on the matrix left (hints only: Ctx::ov_prior_q16 ...)
struct OvHints { uint32_t prior_q16 = 0, slab_q16 = 0; bool tiers_known = false, tier_used[NUM_TIERS] = {false, false, false, false, false, false}, sort_used[2] = {false, false}; };
// phase 0: the whole call.  1: the first half of a sharded call with mirror exchange (seed_matrix_begin): global pair ownership, no finalize.  2: the same,
// only queued (seed_matrix_send): every tier is launched, nothing is read back.  row_lo / row_hi: the window, resolved (Ctx::window).  pass: 1, 2, ...
// tmp_cap: the staging capacity in records, 0 = not chosen yet (then free_bytes — the device's free memory — and workspace_hint_bytes choose it)
struct OvInput {
    int64_t M = 0, N = 0, Z = 0, row_lo = 0, row_hi = 0, max_row_nnz = 0, max_col_nnz = 0;
    uint32_t fbits = 1, s_stride = 0, lpc_log2 = 0;      // (s_stride: padded column stride in entries, 0 = CSC columns)
    bool pos16 = false, use_ell = false, csr_hints = false, csr_inline = false, csr_suffix = false, have_row_order = false;
    int num_cus = 256;
    OvOptions opt;
    OvHints hints;
    int phase = 0, pass = 1;
    int64_t tmp_cap = 0, free_bytes = 0, workspace_hint_bytes = 0;
};

// ---- output -----------------------------------------------------------------------------------------------------------------------------
struct OvLaunch { int row = -1, grid = 0, block = 0; size_t lds = 0; };      // a row of OV_ROWS with its grid and LDS bytes worked out
// the finalize pass (row pointers, mirror, per-row sorts): grids, and which of the two wide-row sorts are launched
struct OvFinPlan {
    int64_t nrows = 0;
    bool slabs = false, scan_rowptr = false, narrow = false;      // the rows hold slab entries (k_row_counts folds them) | row pointers by k_row_counts + scan (M + 1 > 2^17) | no row can be wider than FIN_WAVE2_MAX
    int slab_fold_blocks = 0, rowptr_blocks = 0, row_blocks = 0, bucket_blocks = 0, huge_blocks = FIN_HUGE_BLOCKS;
    uint64_t sort_stride = 2;
    uint32_t sorts = 0;      // launched: bit 0 k_finalize_bucket, bit 1 k_finalize_huge
};
struct OvPlan {
    int64_t nrows = 0;
    bool geom_off = false;      // option "ov_generic" = 2
    bool whole = false, ell = false, forced = false;      // the window is the whole matrix | padded columns | an option forces the general kernel ("ov_generic", "dk", "tune3/4/5/7")
    uint32_t half = 0, pos_mask = 0, hint_mask = 0, suffix = 0, inl = 0;
    bool row_order = false, hints_used = false;
    bool pay = false, pay16 = false;
    OvFamily family = OV_S32;
    int dk = 1;
    bool spec = false, spec_geom = false;      // the reads-path instantiation runs | ... with table size and column geometry compiled in (ov_spec_geom_ok)
    uint32_t s_stride = 0, lpc_log2 = 0, fbits = 0;      // the column geometry of A the kernels run with (OvInput's)
    uint32_t min_tier = 0, qblk_log2 = 0, prior_q16 = 16384, use_feedback = 1, max_col = 1;
    unsigned long long fb_enough = 0;
    uint32_t nsample = 0, sstep = 1;
    bool slab_on = false; int64_t slab_cap = 0; uint32_t slab_prior_q16 = 0;
    uint64_t gstride = 2; int spill_blocks = 64;
    int64_t slack = 0, tmp_cap = 0, b_cap = 0;
    bool mir16 = false;      // staged and mirrored entries are 16-byte words (positions fit 16 bits), not 32-byte records
    uint32_t tier_limit[NUM_LDS_TIERS] = {0, 0, 0, 0, 0};
    OvLaunch tier[NUM_TIERS], sample;      // sample.row < 0: no sample
    int tmax = NUM_TIERS;
    uint32_t launched = 0;      // bit t: tier t is launched this pass
    int zero_blocks_max = 0, classify_blocks = 0;
    OvFinPlan fin;      // phase 0's finalize
};

// The reads-path instantiation of the numeric kernel (OvSpecParams) runs a call whose every switch has the value that instantiation fixes: padded columns
// with inline partners and ownership hints, one triangle + mirror over the whole matrix in one call, 32-bit accumulators carrying posT, 16-byte records,
// the gather depth of inline rows.  Anything else — both triangles, CSC columns, 64-bit accumulators, 32-byte records, the dense path, windows and
// shards, a forced gather depth or tier (option "dk", "tune3" .. "tune5", "tune7"), option "ov_generic" (A/B) — takes the general kernel.
inline bool ov_spec_ok(const OvPlan &p)
{
    return !p.forced && p.dk == 0 && !p.pay && (p.pay16 ? 1u : 0u) == ov_spec::pay16 && p.ell && p.half == ov_spec::half && p.hint_mask == ov_spec::hint_mask &&
           p.pos_mask == ov_spec::pos_mask && p.inl == ov_spec::inl && (p.mir16 ? 1u : 0u) == ov_spec::rec16 && p.suffix == ov_spec::suffix && !p.row_order &&
           p.qblk_log2 == ov_spec::qblk_log2 && p.whole;
}

// The compiled-geometry variant of that instantiation (table size, claim limit, column stride, lanes per row entry and fbits are constants of the kernel)
// runs a reads-path call whose columns have the geometry it fixes; every other stride (4, 16, 24, ...) and option "ov_generic" = 2 (A/B) keep the
// run-time-geometry instantiation.
inline bool ov_spec_geom_ok(const OvPlan &p)
{
    return ov_spec_ok(p) && !p.geom_off && p.s_stride == ov_spec::geom_stride && p.lpc_log2 == ov_spec::geom_lpc_log2 && p.fbits == ov_spec::geom_fbits;
}

inline OvLaunch ov_launch_of(int row, bool pay16, int num_cus, int dense_wgs, int spill_blocks)
{
    const OvTierRow &r = OV_ROWS[row];
    OvLaunch l;
    l.row = row; l.block = r.block; l.lds = ov_row_lds(r, pay16);
    l.grid = r.cu_factor == OV_GRID_SPILL ? spill_blocks : num_cus * (r.cu_factor == OV_GRID_DENSE_WGS ? dense_wgs : r.cu_factor);
    return l;
}

// all_sorts: launch both wide-row sorts whatever the previous call used (cold calls, repeated passes, the sharded calls' finalize); remote: mirrored
// entries of other ranks are merged (their rows can be wider than this matrix alone makes them)
inline OvFinPlan plan_ov_finalize(const OvInput &in, bool slabs, bool all_sorts, bool remote)
{
    OvFinPlan f;
    const int64_t M = in.M, cus = in.num_cus;
    f.nrows = in.row_hi - in.row_lo;
    f.slabs = slabs;
    f.slab_fold_blocks = slabs && f.nrows > 0 ? (int)((f.nrows + 255) / 256) : 0;
    while (f.sort_stride < (uint64_t)M) f.sort_stride <<= 1;
    f.scan_rowptr = M + 1 > (1 << 17);
    f.rowptr_blocks = (int)(f.scan_rowptr ? (M + 1 + 255) / 256 : (M + 1 + RP_TILE - 1) / RP_TILE);
    if (f.nrows <= 0) return f;
    f.row_blocks = (int)std::min<int64_t>((f.nrows + 3) / 4, cus * 32);
    // (a row of B holds at most min(longest row of A x longest column, reads) entries: the sorts for wider rows are not launched for a matrix that cannot have them)
    f.narrow = in.opt.tune4 != 2 && !remote &&
               std::min<uint64_t>((uint64_t)std::max<int64_t>(in.max_row_nnz, 1) * (uint64_t)std::max<int64_t>(in.max_col_nnz, 1), (uint64_t)M) <= (uint64_t)FIN_WAVE2_MAX;
    f.bucket_blocks = (int)std::min<int64_t>(f.nrows, cus * 4);
    if (!f.narrow && (all_sorts || in.hints.sort_used[0])) f.sorts |= 1u;
    if (!f.narrow && (all_sorts || in.hints.sort_used[1])) f.sorts |= 2u;
    return f;
}

// B is symmetric up to exchanging the two positions of every seed (exactly: the canonical seeds are min / max over a cross product of
// positions per shared k-mer): a pair of rows of this context's window is accumulated on its smaller row only and the surviving
// entries are mirrored into the partner's row afterwards (k_mirror) — half the accumulator updates, tables half as full.
// (rows with inline partners hold one triangle's pairs only: "no_symmetry" counts when A is built)
inline bool ov_one_triangle(const OvInput &in) { return in.phase >= 1 || !in.opt.no_symmetry || in.csr_inline; }

// HBM spill tables: 4 x gstride u32 per workgroup, twice the reads (load factor <= 1/2), at most 4 GB of them
struct OvSpill { uint64_t gstride; int blocks; };
inline OvSpill ov_spill_tables(int64_t M, int num_cus)
{
    OvSpill s{2, 0};
    while (s.gstride < 2ull * (uint64_t)(M > 1 ? M : 1)) s.gstride <<= 1;
    s.blocks = (int)((4ull << 30) / (20ull * s.gstride));
    s.blocks = s.blocks < 64 ? 64 : (s.blocks > num_cus * 2 ? num_cus * 2 : s.blocks);
    return s;
}

// plan_ov, part 1: the HBM spill tables, the staging area and the output
inline void ov_plan_capacities(const OvInput &in, OvPlan &p)
{
    const int64_t M = in.M, Z = in.Z;
    const bool half = ov_one_triangle(in);
    const OvSpill sp = ov_spill_tables(M, in.num_cus);
    p.gstride = sp.gstride; p.spill_blocks = sp.blocks;
    p.slack = ov_stage_slack(in.num_cus);
    p.tmp_cap = in.tmp_cap;
    if (p.tmp_cap == 0) {
        if (in.workspace_hint_bytes > 0) p.tmp_cap = in.workspace_hint_bytes / (int64_t)STAGE_REC_BYTES;
        else {
            // nnz(B) <= products / 2 and, on every read set seen so far, < nnz(A) / 4: start from nnz(A) (bounded by half the free memory)
            const int64_t budget = (int64_t)((size_t)in.free_bytes / 2 / (STAGE_REC_BYTES + (half ? 2 * (24 + 32) : 24)));
            p.tmp_cap = std::min<int64_t>(std::max<int64_t>(half ? Z / 2 : Z, 1 << 16) + p.slack, std::max<int64_t>(budget, 1024));
        }
        if (p.tmp_cap < 1024) p.tmp_cap = 1024;
    }
    p.b_cap = half ? 2 * p.tmp_cap : p.tmp_cap;      // the output cannot be larger than what was staged (and mirrored)
}

// part 2: the switches of the kernels, the kernel family, the gather depth, whether the reads-path instantiation runs
inline void ov_plan_switches(const OvInput &in, OvPlan &p)
{
    const OvOptions &o = in.opt;
    const int64_t Z = in.Z, nrows = p.nrows;
    p.max_col = (uint32_t)(in.max_col_nnz > 0 ? in.max_col_nnz : 1);
    p.half = in.phase >= 1 ? 2u : (ov_one_triangle(in) ? 1u : 0u);      // 2: a pair is accumulated on ONE of its two rows wherever the other row lives (its rank gets the mirrored entry by exchange)
    p.pos_mask = csr_pos_mask(in.csr_suffix, in.csr_hints);
    p.hint_mask = !in.csr_hints ? 0u : (p.half == 2u ? 1u << 30 : (p.half == 1u ? 1u << 31 : 0u));
    // (the dense path: one triangle per window, partners outside the window kept — its candidate hand-out knows no other rule.  Both triangles
    //  ("no_symmetry") and the mirror exchange between ranks (half == 2: the parity rule over all ranks) take the general path, which reads the
    //  same entries through pos_mask)
    p.suffix = in.csr_suffix && p.half == 1u ? 1u : 0u;
    p.inl = in.csr_inline ? 1u : 0u;
    p.row_order = p.suffix && in.have_row_order;
    p.hints_used = p.hint_mask != 0u || p.suffix != 0u || in.csr_inline;      // (entries that fetch no column do not see its length: the product count comes from the build of A)
    p.prior_q16 = in.hints.prior_q16 ? in.hints.prior_q16 : 16384u;      // distinct partners per row entry: 1/4 until measured
    p.use_feedback = in.hints.prior_q16 ? 0u : 1u;
    p.fb_enough = (unsigned long long)std::min<int64_t>(std::max<int64_t>(Z / 32, 1 << 16), 1 << 23);
    p.pay = in.pos16 && !o.no_pay;
    // where the positions AND every row's product sequence numbers (rank in the row << fbits | place in the column) fit 16 bits — every read set of
    // ~10 kb reads — the extremes live in 32-bit words that carry posT (posQ is looked up in the row entry the sequence number names): the 2048-slot tier
    // then needs 37 KB of table + 16 KB of rings per 512-lane workgroup instead of 53 + 24.5: THREE rows per CU in flight instead of two (the kernel waits for
    // memory 69 % of its time: profiles/r04_summary.json), at the same 72-78 VGPRs.  Option "tune3" = 1 keeps the 64-bit accumulators (A/B).
    p.pay16 = p.pay && in.use_ell && !in.csr_suffix && o.tune3 != 1 && ((uint64_t)in.max_row_nnz << in.fbits) <= 65536ull;
    if (p.pay16) p.pay = false;
    p.family = p.suffix ? OV_DENSE : p.pay ? OV_PAY : OV_S32;      // (dense matrices: the LDS tiers with 64-bit accumulators run the dense path; suffix implies pay)
    p.mir16 = in.pos16 && !o.mir32;
    // a large matrix's rows start on the 2048-slot tier at least (three rows per CU with pay16): the two smaller tiers would receive a percent of the rows and cost a
    // ~60 us launch each — 6.48 -> 6.3x ms on config 3; small matrices keep them (their rows ARE small); option "tune4" = 1: every tier (A/B)
    p.qblk_log2 = o.tune5 > 0 ? (uint32_t)std::min<int64_t>(o.tune5 - 1, 12) : 0u;      // ("tune5" = log2 + 1.  Measured on config 5 at 1/25 — label-ordered queue, blocks of 32 / 128 / 512 places per XCD: 8.66-8.74 against 8.74-8.77 ms: nothing; single places stay)
    p.min_tier = (p.pay16 && nrows >= 65536 && Z / nrows >= 1024 && o.tune4 != 1) ? 2u : 0u;      // (long rows only: a 512-lane workgroup on a row of 75 entries would idle)
    if (o.tune7 >= 1 && o.tune7 <= NUM_TIERS) p.min_tier = (uint32_t)(o.tune7 - 1);      // ("tune7" = tier + 1: every row starts there at least; 6 = the HBM-table tier for all of them — what the spill tier costs when forced, bench.py)
    // gather trips per iteration of the padded-column loop: 1 (DK = 0) where the rows mostly carry their products inline — columns of 2-3
    // reads, 15 %-error reads: 6.49 -> 6.27 ms on config 3 —, 2 (DK = 1) otherwise (columns of ~7 reads at 5 % error lose 4 % with one trip);
    // the option "dk" (0, 1, 2, 4) overrides
    p.dk = o.dk >= 0 ? o.dk : ((in.csr_inline && in.N > 0 && Z < 3 * in.N) ? 0 : 1);
    p.spec = ov_spec_ok(p);      // (the reads path: its switches compiled into the kernel)
    p.spec_geom = ov_spec_geom_ok(p);      // (... and its geometry)
}

// part 3: the sample of a cold call and the mirror slabs
inline void ov_plan_sample_slabs(const OvInput &in, OvPlan &p)
{
    const OvOptions &o = in.opt;
    const int64_t M = in.M, nrows = p.nrows;
    // A cold call on a matrix of some size computes a SAMPLE of its rows first (every sstep-th row, on the 4096-slot tier): what they find
    // — distinct partners per row entry — picks the starting tier of all the others, instead of a guess that sends most rows of a
    // 15 %-error read set to a tier too small (an abandoned attempt or a forwarding each: 0.9 ms of a 14.7 ms call on the 200 k-read set).
    const bool sampling = p.use_feedback && nrows >= 8192 && !o.no_sample;
    p.nsample = sampling ? (uint32_t)OV_SAMPLE_ROWS : 0u; p.sstep = sampling ? (uint32_t)(nrows / OV_SAMPLE_ROWS) : 1u;
    // mirror slabs (spgemm.hip): one call on the window, 16-byte records, a ratio to size them by — a sample of this call's rows, an earlier call's
    // measurement, or the test hook
    p.slab_prior_q16 = o.slab_q16 > 0 ? (uint32_t)o.slab_q16 : in.hints.slab_q16;
    p.slab_on = in.phase == 0 && p.half == 1u && p.mir16 && !o.no_slab && nrows > 0 && (sampling || p.slab_prior_q16 != 0u);
    if (p.slab_on) {
        p.slab_cap = std::min<int64_t>(p.tmp_cap + (int64_t)SLAB_PAD * nrows, 0xFFFF0000ll);
        // (the fill word of a row is slab end << 32 | next free entry, bumped once per image — also by those that find the slab full: a row receives
        //  at most M images, so the low half cannot carry into the end as long as the slab area + M stays below 2^32)
        if (p.slab_cap + M >= 0xFFFFFFFFll) p.slab_cap = std::max<int64_t>(0xFFFFFFFFll - M - 1, 0);
        if (p.slab_cap <= (int64_t)SLAB_PAD * nrows + 1) p.slab_on = false;      // (no room left for slabs under that bound: tickets + k_mirror)
    }
}

// part 4: the tiers' rows with their geometry, the highest tier any row can reach, the tiers launched this pass
inline void ov_plan_tiers(const OvInput &in, OvPlan &p)
{
    const OvOptions &o = in.opt;
    const int64_t M = in.M, nrows = p.nrows;
    // the tiers' rows, and from the rows' own workgroup sizes the claimed slots at which a row abandons a tier: min(3T/4, T - block) - 1 (a lane
    // overshoots by at most one claim: Table::insert_lds)
    for (int t = 0; t < NUM_TIERS; ++t) p.tier[t] = ov_launch_of(ov_row_of(p.family, t, (int)o.dense_up), p.pay16, in.num_cus, o.dense_wgs, p.spill_blocks);
    for (int t = 0; t < NUM_LDS_TIERS; ++t)
        p.tier_limit[t] = ov_tier_limit(OV_ROWS[p.tier[t].row].tbits, p.tier[t].block);
    if (p.nsample) p.sample = p.tier[OV_SAMPLE_TIER];
    // the highest tier ANY row of this matrix can reach: a row's distinct partners <= min(its entries x the longest column, reads), the tier that holds
    // twice that is guaranteed to fit it and k_classify_direct never starts a row above it.  A cold call on a small matrix launched five tiers
    // nobody could queue on (~5 us each, dependent: hifi-half 0.59 -> 0.53 ms with the finalize's counterpart).  (Still under the `missed` check of ov_settle.)
    // (a repeated pass launches every tier: whatever the first one missed, it cannot miss it again for want of a launch)
    if (o.tune4 != 2 && in.pass == 1) {
        const uint64_t ubm = std::min<uint64_t>((uint64_t)std::max<int64_t>(in.max_row_nnz, 1) * (uint64_t)p.max_col, (uint64_t)(uint32_t)M);
        const int gmax = ubm <= 1 ? 1 : 64 - __builtin_clzll(2 * ubm - 1);
        p.tmax = gmax <= LDS_TBITS0 ? 0 : gmax - LDS_TBITS0;
        p.tmax = std::max(p.tmax, (int)p.min_tier);
        if (p.suffix) p.tmax = std::max(p.tmax, (int)o.dense_up);
    }
    const bool all_tiers = !in.hints.tiers_known || in.phase == 2;
    for (int t = 0; t < NUM_TIERS; ++t)
        if (nrows > 0 && (all_tiers || in.hints.tier_used[t]) && t <= p.tmax) p.launched |= 1u << t;
}

inline OvPlan plan_ov(const OvInput &in)
{
    OvPlan p;
    const OvOptions &o = in.opt;
    const int64_t cus = in.num_cus, nrows = in.row_hi - in.row_lo;
    p.nrows = nrows;
    p.whole = in.row_lo == 0 && in.row_hi == in.M;
    p.ell = in.use_ell;
    p.s_stride = in.s_stride; p.lpc_log2 = in.lpc_log2; p.fbits = in.fbits; p.geom_off = o.spec_rt_geom;
    p.forced = o.ov_generic || o.dk >= 0 || o.tune3 != 0 || o.tune4 != 0 || o.tune5 != 0 || o.tune7 != 0;
    ov_plan_capacities(in, p);
    ov_plan_switches(in, p);
    ov_plan_sample_slabs(in, p);
    ov_plan_tiers(in, p);
    p.zero_blocks_max = in.num_cus * 8;
    p.classify_blocks = nrows > 0 ? (int)std::min<int64_t>((nrows + 255) / 256, cus * 4) : 0;
    p.fin = plan_ov_finalize(in, p.half == 1u && p.mir16 && p.slab_on, !in.hints.tiers_known, false);
    return p;
}

// what a repeated pass changes: staging as large as the cursor says was needed (every row drew its space even when it did not fit), and nothing of
// what earlier calls knew about tiers and sorts — plan_ov then launches every tier and both sorts (pass > 1 lifts tmax)
inline OvInput ov_next_pass(const OvInput &in, const OvPlan &p, bool overflow, unsigned long long cursor)
{
    OvInput n = in;
    n.pass = in.pass + 1;
    n.tmp_cap = overflow ? (int64_t)cursor + p.slack : p.tmp_cap;
    n.hints.tiers_known = false;
    return n;
}

// what a finished call leaves for the next one: the tiers and sorts that got rows; mirrored entries per row entry of A (whole-matrix calls that merged
// nothing from other ranks); the measured distinct-partner / row-entry ratio + 25 %, replacing the old one when it differs by more than a tenth
struct OvMeasured { int64_t Z = 0, nnz = 0, ndiag = 0, extra_nnz = 0; bool whole = false; unsigned long long fb_claims = 0, fb_ub = 0; unsigned int tier_count[NUM_TIERS] = {0, 0, 0, 0, 0, 0}, fin_count[2] = {0, 0}; };
inline OvHints ov_next_hints(const OvHints &old, const OvMeasured &m)
{
    OvHints h = old;
    for (int t = 0; t < NUM_TIERS; ++t) h.tier_used[t] = m.tier_count[t] > 0;
    h.tiers_known = true;
    h.sort_used[0] = m.fin_count[0] > 0; h.sort_used[1] = m.fin_count[1] > 0;
    if (m.whole && m.Z > 0 && m.extra_nnz == 0) {
        const double r = 0.5 * (double)(m.nnz - m.ndiag) / (double)m.Z * 65536.0;
        h.slab_q16 = r < 1.0 ? 1u : (r > 4.0e9 ? 4000000000u : (uint32_t)r);
    }
    if (m.fb_ub > 0) {
        const double r = 1.25 * (double)m.fb_claims / (double)m.fb_ub * 65536.0;
        const uint32_t q = r < 64.0 ? 64u : (r > 4.0e9 ? 4000000000u : (uint32_t)r);
        if (old.prior_q16 == 0 || q > old.prior_q16 + old.prior_q16 / 10 || q + old.prior_q16 / 10 < old.prior_q16) h.prior_q16 = q;
    }
    return h;
}

}  // namespace elba
