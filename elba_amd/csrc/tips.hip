// tips.hip — clipping dead-end tips from the string graph (elba_clip_tips): not in the reference, whose GenerateContigs drops every read of
// degree > 2 with its edges, so that one stray read hanging off a good path cuts it into three contigs.
//
// Input and output: the S that tr.hip leaves on the context (tr_out_*), column-major, both triangles.  The rule is stated on columns alone:
// deg(v) = length of column v, the neighbours of v = the rows of column v (ascending).  One ROUND, on the degrees as the round finds them:
//   dead end   a read of degree 1
//   walk       v1 = a dead end, v2 = its neighbour; from a read vi (i > 1) of degree 2 the walk goes on to the smaller row of column vi
//              that is not v(i-1) (on a symmetric S: the neighbour it did not come from).  It ends at the first read of degree >= 3 (the
//              anchor b: v1 .. vt is a tip of t reads), at a read of degree 1 or 0 (a plain path: no tip) or when read max_tip_reads + 1
//              would join the chain (too long: no tip)
//   sparing    T(b) = tips anchored at b.  T(b) < deg(b): all of them go.  T(b) >= deg(b) (a star of short chains): none goes, b is a
//              spared anchor, counted once
//   removal    every entry whose row or column is a removed read leaves S; the others keep their values and their order
// Everything a round decides is read from tables frozen when it starts (ptr, ntips) and what it writes are sets (removed) and sums:
// the order in which the lanes run does not show in the result.
//
//   k_tip_begin     column pointers of the round's S from its column ids (nnz read on the device), ntips = 0, anchor = none
//   k_tip_walk      one lane per read; a lane on a dead end walks at most max_tip_reads steps; at an anchor it records anchor[v1] and does
//                   one atomicAdd on ntips[anchor]
//   k_tip_mark      a lane whose dead end has an anchor with ntips < deg walks again: removed[vi] = 1 (atomicExch: the winner counts the
//                   read and sets flag bit 2); a lane on a read with deg >= 3 and ntips >= deg counts it as spared
//   keep flags, scan, scatter: the compaction of sg_rounds.hpp
//
// Rounds without host synchronisation, in batches of SG_BATCH with one synchronisation per batch: the protocol of sg_rounds.hpp.  The
// rule's part of it: every kernel here returns at once when the round before removed nothing, and k_tip_mark adds the reads it removed to
// *sg_removed_slot(st, r).
//
// Bounds: every index into rows / cols is below the round's nnz (ptr built from n), every read index below M (rows and cols of S are; a
// walk also tests cur < M), a walk reads rows only from a column of length 1 or 2; the compaction's bounds are in sg_rounds.hpp.
// Bytes (algorithmic) per round that removes something: the compaction's (sg_rounds.hpp: 52 bytes per entry read, 52 per kept entry
// written, + 28) and M x 16 for pointers, ntips, anchors.
#include "sg_rounds.hpp"

namespace elba {

namespace {

constexpr uint32_t TP_NONE = 0xffffffffu;
constexpr int TP_THREADS = 256;                 // threads of every kernel here
constexpr int TP_TILE = 256;                    // entries of S one workgroup of the compaction's scatter moves (sg_rounds.hpp)
// (both spelled out: every version of tests/test_gpu_tips.py before the one that asks rounds_util for SG_TILE reads them from this file)
static_assert(TP_THREADS == SG_THREADS && TP_TILE == SG_TILE, "the compaction is sg_rounds.hpp's");
// st[]: 0 dead ends (first round), 1 tips, 2 reads removed, 3 spared anchors; the protocol's slots: sg_rounds.hpp
enum { TP_DEAD = 0, TP_TIPS = 1, TP_READS = 2, TP_SPARED = 3 };
static_assert(TP_SPARED < SG_LIVE, "the rule's counters lie in front of the protocol's");

__global__ void k_tip_begin(const int64_t *cols, const u64 *st, int r, uint32_t M, uint32_t *ptr, uint32_t *ntips, uint32_t *anchor)
{
    if (!sg_live(st, r)) return;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (int64_t)M) { ntips[i] = 0; anchor[i] = TP_NONE; }
    sg_col_ptrs(cols, sg_nnz(st, r), M, i, ptr);
}

__global__ void k_tip_walk(const uint32_t *ptr, const int64_t *rows, u64 *st, int r, uint32_t maxt, uint32_t M, uint32_t *ntips, uint32_t *anchor)
{
    if (!sg_live(st, r)) return;
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    bool dead = false, tip = false;
    if (v < M) {
        const uint32_t s = ptr[v];
        if (ptr[v + 1] - s == 1) {
            dead = true;
            uint32_t prev = v, cur = (uint32_t)rows[s], t = 1;          // t reads in the chain so far
            while (cur < M) {
                const uint32_t cs = ptr[cur], d = ptr[cur + 1] - cs;
                if (d >= 3) { anchor[v] = cur; atomicAdd(&ntips[cur], 1u); tip = true; break; }
                if (d != 2 || t == maxt) break;                         // the other end of a path, or a chain longer than max_tip_reads
                const uint32_t nx = sg_walk_next(rows, cs, prev);
                prev = cur; cur = nx; ++t;
            }
        }
    }
    sg_count(&st[TP_DEAD], dead && r == 0);
    sg_count(&st[TP_TIPS], tip);
}

__global__ void k_tip_mark(const uint32_t *ptr, const int64_t *rows, u64 *st, int r, uint32_t M, const uint32_t *ntips, const uint32_t *anchor,
                           uint32_t *removed, uint8_t *flags)
{
    if (!sg_live(st, r)) return;
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    bool spared = false;
    if (v < M) {
        const uint32_t d = ptr[v + 1] - ptr[v];
        spared = d >= 3 && ntips[v] >= d;
        const uint32_t b = anchor[v];
        if (b != TP_NONE && ntips[b] < ptr[b + 1] - ptr[b]) {           // the walk of k_tip_walk again: it reached b within max_tip_reads steps
            uint32_t prev = TP_NONE, cur = v, cnt = 0;
            while (cur != b) {
                if (atomicExch(&removed[cur], 1u) == 0) { ++cnt; flags[cur] = (uint8_t)(flags[cur] | 4u); }
                const uint32_t cs = ptr[cur];
                const uint32_t nx = sg_walk_next(rows, cs, prev, ptr[cur + 1] - cs == 1);
                prev = cur; cur = nx;
            }
            if (cnt) { atomicAdd(&st[TP_READS], (u64)cnt); atomicAdd(sg_removed_slot(st, r), (u64)cnt); }
        }
    }
    sg_count(&st[TP_SPARED], spared);
}

}  // namespace

void stage_clip_tips(Ctx &c, const elba_tip_cfg *cfgp)
{
    const elba_tip_cfg &cfg = sg_enter(c, EV_CLIP_TIPS, cfgp);
    ELBA_REQUIRE(cfg.max_tip_reads >= 1 && cfg.max_tip_reads <= 65535, ELBA_ERR_INVALID_ARG, "clip_tips: max_tip_reads outside 1 .. 65535");
    ELBA_REQUIRE(cfg.rounds >= 1 && cfg.rounds <= SG_MAX_ROUNDS, ELBA_ERR_INVALID_ARG, "clip_tips: rounds outside 1 .. 64");
    ELBA_REQUIRE(!cfg.reserved[0] && !cfg.reserved[1], ELBA_ERR_INVALID_ARG, "clip_tips: reserved words must be 0");
    const int64_t M = c.tr_M, n0 = c.tr_nnz;
    sg_require_32bit(EV_CLIP_TIPS, M < 0xffffffffll && n0 < 0xfffffffell);
    elba_tip_stats st = sg_stats_begin<elba_tip_stats>(c);
    st.rounds_run = 1;
    if (M == 0 || n0 == 0) { accepted(c.v, EV_CLIP_TIPS); done(c.v, EV_CLIP_TIPS); c.tp.stats = st; return; }      // no entry: no dead end, the one round removes nothing
    // every buffer of the launch sequence before the first launch
    sg_reserve(c, M, n0);
    c.tp.ntips.reserve((size_t)(M + 1) * 4); c.tp.anchor.reserve((size_t)(M + 1) * 4);
    const SgCall w(c);
    uint32_t *ntips = c.tp.ntips.as<uint32_t>(), *anchor = c.tp.anchor.as<uint32_t>();
    accepted(c.v, EV_CLIP_TIPS);                                // S changes under the contigs of the old one, and is itself invalid until the counters are back:
                                                                // a call that fails below leaves no S rather than one in the wrong buffer
    u64 h[SG_ST];
    const int moves = sg_run_rounds(w, cfg.rounds, h, [&](int r, const int64_t *rows, const int64_t *cols) {
        hipLaunchKernelGGL(k_tip_begin, dim3(w.nbB), dim3(TP_THREADS), 0, w.s, cols, w.st, r, (uint32_t)M, w.ptr, ntips, anchor);
        hipLaunchKernelGGL(k_tip_walk, dim3(w.nbM), dim3(TP_THREADS), 0, w.s, w.ptr, rows, w.st, r, (uint32_t)cfg.max_tip_reads, (uint32_t)M, ntips, anchor);
        hipLaunchKernelGGL(k_tip_mark, dim3(w.nbM), dim3(TP_THREADS), 0, w.s, w.ptr, rows, w.st, r, (uint32_t)M, ntips, anchor, w.removed, w.flags);
    });
    done(c.v, EV_CLIP_TIPS);
    st.dead_ends = (int64_t)h[TP_DEAD]; st.tips = (int64_t)h[TP_TIPS]; st.reads_removed = (int64_t)h[TP_READS]; st.spared_anchors = (int64_t)h[TP_SPARED];
    st.rounds_run = moves < cfg.rounds ? moves + 1 : cfg.rounds;
    sg_stats_end(c, st);
    c.tp.stats = st;
}

}  // namespace elba
