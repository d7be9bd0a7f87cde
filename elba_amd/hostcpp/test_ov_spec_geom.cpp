// test_ov_spec_geom — walks the selection of the compiled-geometry reads-path kernel (csrc/ov_plan.hpp: ov_spec_geom_ok) without the library: the column
// strides that take it and those that keep the run-time geometry, every knob that turns the reads path off, the A/B value of option "ov_generic", and
// the claim limits the kernels compile in (ov_tier_limit) against the plan's tier_limit[] and against the literals.
// Prints one line per failed check and "ok <checks>" at the end (tests/test_ov_spec_geom_cpu.py reads it); exit status 1 if a check failed.
#include "../csrc/ov_plan.hpp"
#include <cstdio>

using namespace elba;

static int g_checks = 0, g_failed = 0;
#define CHECK(cond, ...) do { ++g_checks; if (!(cond)) { ++g_failed; printf("FAILED %s:%d %s | ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } while (0)

// what matrix.hip (choose_column_store) makes of a longest column of `mc` entries, mc <= 64: stride, lanes per row entry (log2), fbits
struct Geom { uint32_t stride, lb, fb; };
static Geom column_store(uint32_t mc)
{
    Geom g{mc <= 4 ? 4u : (mc + 7u) & ~7u, 1, 2};
    while ((2u << g.lb) < g.stride) ++g.lb;
    while ((1u << g.fb) < g.stride) ++g.fb;
    return g;
}

// a matrix built from 15 %-error reads, multiplied whole (the shape test_ov_plan.cpp calls reads_in), its longest column `mc`
static OvInput reads_in(uint32_t mc)
{
    OvInput in;
    in.M = 2000; in.N = 900000; in.Z = 2100000; in.row_lo = 0; in.row_hi = in.M; in.max_row_nnz = 1000; in.max_col_nnz = mc;
    const Geom g = column_store(mc);
    in.fbits = g.fb; in.s_stride = g.stride; in.lpc_log2 = g.lb;
    in.pos16 = true; in.use_ell = true; in.csr_hints = true; in.csr_inline = true; in.num_cus = 256; in.free_bytes = 200ll << 30;
    return in;
}

int main()
{
    // the strides
    for (uint32_t mc : {1u, 2u, 4u, 5u, 6u, 7u, 8u, 9u, 16u, 33u, 40u}) {
        const OvInput in = reads_in(mc);
        const OvPlan p = plan_ov(in);
        const bool eight = mc >= 5 && mc <= 8;
        CHECK(in.s_stride == (mc <= 4 ? 4u : mc <= 8 ? 8u : mc <= 16 ? 16u : 40u), "longest column %u: stride %u", mc, in.s_stride);
        CHECK(p.spec, "longest column %u: the reads path", mc);
        CHECK(p.spec_geom == eight && ov_spec_geom_ok(p) == eight, "longest column %u: compiled geometry %d", mc, (int)p.spec_geom);
        if (p.spec_geom) CHECK(p.s_stride == ov_spec::geom_stride && p.lpc_log2 == ov_spec::geom_lpc_log2 && p.fbits == ov_spec::geom_fbits && p.s_stride == 8u && p.lpc_log2 == 2u && p.fbits == 3u, "longest column %u: the constants", mc);
    }
    { const Geom g4 = column_store(4), g8 = column_store(8), g16 = column_store(16), g40 = column_store(40);
      CHECK(g4.stride == 4 && g4.lb == 1 && g4.fb == 2 && g8.stride == 8 && g8.lb == 2 && g8.fb == 3 && g16.stride == 16 && g16.lb == 3 && g16.fb == 4 && g40.stride == 40 && g40.lb == 5 && g40.fb == 6, "column stores"); }
    // a stride of 8 with other lanes or fbits (not what choose_column_store makes, but what the predicate must refuse)
    { OvInput in = reads_in(8); in.lpc_log2 = 3; CHECK(plan_ov(in).spec && !plan_ov(in).spec_geom, "lanes");
      in = reads_in(8); in.fbits = 4; CHECK(plan_ov(in).spec && !plan_ov(in).spec_geom, "fbits");
      in = reads_in(8); in.s_stride = 0; CHECK(!plan_ov(in).spec_geom, "no stride"); }
    // every knob that turns the reads path off turns the compiled geometry off with it
    { int n = 0;
      auto off = [&](const char *what, OvInput in) { const OvPlan p = plan_ov(in); CHECK(!p.spec && !p.spec_geom && !ov_spec_geom_ok(p), "%s: general kernel", what); ++n; };
      OvInput in;
      in = reads_in(8); in.opt.ov_generic = true; off("ov_generic", in);
      in = reads_in(8); in.opt.no_symmetry = true; in.csr_inline = false; off("no_symmetry", in);
      in = reads_in(8); in.opt.no_pay = true; off("no_pay", in);
      in = reads_in(8); in.opt.tune3 = 1; off("tune3", in);
      in = reads_in(8); in.opt.mir32 = true; off("mir32", in);
      in = reads_in(8); in.use_ell = false; in.s_stride = 0; off("no_ell", in);
      in = reads_in(8); in.csr_hints = false; off("no_hints", in);
      in = reads_in(8); in.csr_inline = false; off("no_inline", in);
      in = reads_in(8); in.pos16 = false; off("positions beyond 16 bits", in);
      for (int dk : {0, 1, 2, 4}) { in = reads_in(8); in.opt.dk = dk; off("dk", in); }
      for (int v : {1, 2}) { in = reads_in(8); in.opt.tune4 = v; off("tune4", in); }
      for (int v : {3, 6}) { in = reads_in(8); in.opt.tune7 = v; off("tune7", in); }
      in = reads_in(8); in.opt.tune5 = 6; off("tune5", in);
      in = reads_in(8); in.Z = 3 * in.N; off("Z = 3 N: two gather trips", in);
      in = reads_in(8); in.max_row_nnz = 8193; off("sequence numbers beyond 16 bits", in);
      in = reads_in(8); in.row_lo = 1; off("a window", in);
      in = reads_in(8); in.phase = 1; off("a sharded call", in);
      CHECK(n == 22, "cases %d", n); }
    // the A/B value: the reads path stays, with its run-time geometry; nothing else of the plan moves
    { OvInput in = reads_in(8);
      const OvPlan a = plan_ov(in);
      in.opt.spec_rt_geom = true;
      const OvPlan b = plan_ov(in);
      CHECK(a.spec && a.spec_geom && b.spec && !b.spec_geom, "ov_generic = 2: run-time geometry");
      bool same = a.launched == b.launched && a.tmax == b.tmax && a.dk == b.dk && a.pay16 == b.pay16 && a.mir16 == b.mir16 && a.nsample == b.nsample && a.slab_on == b.slab_on && a.tmp_cap == b.tmp_cap && a.min_tier == b.min_tier;
      for (int t = 0; t < NUM_TIERS; ++t) same = same && a.tier[t].row == b.tier[t].row && a.tier[t].grid == b.tier[t].grid && a.tier[t].block == b.tier[t].block && a.tier[t].lds == b.tier[t].lds;
      for (int t = 0; t < NUM_LDS_TIERS; ++t) same = same && a.tier_limit[t] == b.tier_limit[t];
      CHECK(same, "ov_generic = 2: the same plan otherwise");
      in.opt.ov_generic = true; CHECK(!plan_ov(in).spec && !plan_ov(in).spec_geom, "ov_generic wins");
      // "no_sample" and "no_slab" are not among what the instantiation fixes
      in = reads_in(8); in.opt.no_sample = true; in.opt.no_slab = true; CHECK(plan_ov(in).spec_geom, "no_sample, no_slab: still the compiled geometry"); }
    // the claim limits a compiled-geometry kernel holds as a constant: the rows the reads path runs on (32-bit accumulators + the shared 8192-slot row)
    { const OvPlan p = plan_ov(reads_in(8));
      const uint32_t lit[NUM_LDS_TIERS] = {383u, 767u, 1535u, 3071u, 6143u};
      for (int t = 0; t < NUM_LDS_TIERS; ++t) {
          const OvTierRow &r = OV_ROWS[p.tier[t].row];
          CHECK(!r.dense && !r.global && !r.payload && r.tier == t && r.tbits == LDS_TBITS0 + t, "tier %d: a reads-path row", t);
          CHECK(ov_tier_limit(r.tbits, r.block) == p.tier_limit[t] && p.tier_limit[t] == lit[t], "tier %d: limit %u against %u", t, ov_tier_limit(r.tbits, r.block), p.tier_limit[t]);
          const uint32_t T = 1u << r.tbits;
          CHECK(ov_tier_limit(r.tbits, r.block) == std::min(3 * T / 4, T - (uint32_t)r.block) - 1 && p.tier_limit[t] + 1 + (uint32_t)r.block <= T, "tier %d: every lane may overshoot by one claim", t);
          CHECK((4u << r.tbits) <= 0xFFFFu && ((12u << r.tbits) <= 0xFFFFu) == (t <= 3), "tier %d: which arrays the 16-bit offset field of an LDS instruction reaches", t);
          CHECK((T == 4u * (uint32_t)r.block) == (t <= 3), "tier %d: four slots per lane in the sweep", t);
      }
      // (every family's rows state the same expression)
      for (int r = 0; r < OV_NROWS; ++r)
          if (!OV_ROWS[r].global) CHECK(ov_tier_limit(OV_ROWS[r].tbits, OV_ROWS[r].block) + 1 + (uint32_t)OV_ROWS[r].block <= (1u << OV_ROWS[r].tbits), "row %d", r); }
    if (g_failed) { printf("%d of %d checks failed\n", g_failed, g_checks); return 1; }
    printf("ok %d\n", g_checks);
    return 0;
}
