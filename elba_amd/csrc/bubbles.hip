// bubbles.hip — popping simple bubbles in the string graph (elba_pop_bubbles): not in the reference, whose GenerateContigs drops every read
// of degree > 2 with its edges, so that two short chains between the same two reads cut a path into four contigs and lose both end reads.
//
// Input and output: the S that tr.hip leaves on the context (tr_out_*), column-major, both triangles, as for tips.hip.  The rule is stated on
// columns alone: deg(v) = length of column v, the neighbours of v = the rows of column v (ascending).  One ROUND, on the degrees as it finds them:
//   anchor     a read of degree >= 3
//   arm        for an entry z of a column a that is an anchor, whose row v1 has degree 2: the walk of tips.hip from v1, "came from" = a; from
//              vi of degree 2 it goes on to the smaller row of column vi that is not v(i-1).  The first read b of degree >= 3 ends it: v1 ..
//              vt, 1 <= t <= max_arm_reads, is an arm of t reads from a to b — if b > a (the arm is recorded at its smaller anchor; b == a, a
//              chain back to a, is no arm).  A read of degree 0 or 1 ends it too (no arm), and so does read max_arm_reads + 1 (too long)
//   bubble     the arms with the same (a, b), when there are two or more
//   kept arm   the one with the most reads; among those the one with the smallest entry z (= the smallest first read: rows ascend in a column)
//   removal    the reads of every other arm of a bubble go: every entry whose row or column is one of them leaves S, the others keep their
//              values and their order.  An entry a - b itself is no arm and stays
// Everything a round decides is read from tables frozen when it starts (ptr, then arm_end / arm_len, which k_bub_pick only reads) and what it
// writes are sets (removed) and sums: the order in which the lanes run does not show in the result.
//
//   k_bub_begin     column pointers of the round's S from its column ids (nnz read on the device: sg_col_ptrs), arm_end = none, arm_len = 0
//   k_bub_walk      one lane per entry z; if deg(col) >= 3 and deg(row) == 2 the lane walks at most max_arm_reads steps; at an anchor b > col
//                   it writes arm_end[z] = b, arm_len[z] = t and counts an arm.  The first entry of every column of length >= 3 counts an
//                   anchor (first round only)
//   k_bub_pick      one lane per entry that holds an arm: it looks through column a's entries for arms with the same arm_end; it is the kept
//                   arm if none has a larger (arm_len, -z); the kept lane of a group of >= 2 counts a bubble; every other lane walks its arm
//                   again, arm_len reads: removed[vi] = 1 (atomicExch: the winner counts the read and sets flag bit 3), and counts a removed arm
//   keep flags, scan, scatter: the compaction of sg_rounds.hpp
//
// The pick is quadratic per anchor: an arm costs deg(a) reads of arm_end (4 bytes, the same addresses for the lanes of a column, which are
// neighbours: cached) and one of arm_len per arm of its group, so a pair of hubs joined by d arms costs d^2 of each.  The alternative, sorting
// arm records by (a, b, len, z) with prims.hip's radix sort, costs four passes over 16-byte records and two more buffers for every round of
// every call; after the reduction degrees are small (the layout graph of DESIGN 4.12: 3 or 4 at an anchor), so the scan of a column is a
// handful of reads, and the sort would be the larger part of a round.  DESIGN 4.14 has what a hub of 3000 arms costs.
//
// Rounds without host synchronisation, in batches of four with one synchronisation per batch: the protocol of sg_rounds.hpp.  The rule's
// part of it: every kernel here returns at once when the round before removed nothing, and k_bub_pick adds the reads it removed to
// *sg_removed_slot(st, r).
//
// Bounds: a lane works on an entry z < n, the round's nnz; ptr is built from n, so every column range lies in [0, n) and arm_end / arm_len
// (n0 + 1 elements, n <= n0) are read and written below n; every read index is tested below M before ptr is read at it (rows and cols of S
// are; the walks test cur < M again); a walk reads rows only from a column of length 2, at its two entries; k_bub_pick repeats a walk that
// k_bub_walk finished on the same tables, for exactly arm_len steps; removed and flags are written at reads below M; the compaction's bounds
// are in sg_rounds.hpp.
// Bytes (algorithmic) per round: k_bub_begin 8 per entry read (column ids), 8 written (arm_end, arm_len), 4 x M of pointers written;
// k_bub_walk 16 per entry read (row, column id) and the two pointers of its column; k_bub_pick 4 per entry read (arm_end): 36 x nnz + 4 x M,
// the walks and the anchors' columns apart (they touch the arms only).  If the round removes something, the compaction's as well
// (sg_rounds.hpp: 52 bytes per entry read, 52 per kept entry written, + 28).
#include "sg_rounds.hpp"

namespace elba {

namespace {

constexpr uint32_t BB_NONE = 0xffffffffu;
constexpr int BB_THREADS = SG_THREADS;          // threads of every kernel here
// st[]: 0 anchors (first round), 1 arms, 2 bubbles, 3 arms removed, 4 reads removed; the protocol's slots: sg_rounds.hpp
enum { BB_ANCHORS = 0, BB_ARMS = 1, BB_BUBBLES = 2, BB_GONE = 3, BB_READS = 4 };
static_assert(BB_READS < SG_LIVE, "the rule's counters lie in front of the protocol's");

__global__ void k_bub_begin(const int64_t *cols, const u64 *st, int r, uint32_t M, uint32_t *ptr, uint32_t *arm_end, uint32_t *arm_len)
{
    if (!sg_live(st, r)) return;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t n = sg_nnz(st, r);
    if (i < n) { arm_end[i] = BB_NONE; arm_len[i] = 0; }
    sg_col_ptrs(cols, n, M, i, ptr);
}

__global__ void k_bub_walk(const uint32_t *ptr, const int64_t *rows, const int64_t *cols, u64 *st, int r, uint32_t maxt, uint32_t M,
                           uint32_t *arm_end, uint32_t *arm_len)
{
    if (!sg_live(st, r)) return;
    const int64_t z = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t n = sg_nnz(st, r);
    bool anchor = false, arm = false;
    if (z < n) {
        const uint32_t a = (uint32_t)cols[z], v1 = (uint32_t)rows[z];
        if (a < M && v1 < M) {
            const uint32_t as = ptr[a];
            if (ptr[a + 1] - as >= 3) {
                anchor = r == 0 && (int64_t)as == z;                    // once per anchor: at the first entry of its column
                uint32_t prev = a, cur = v1, t = 0;                     // t reads in the chain so far
                while (cur < M) {
                    const uint32_t cs = ptr[cur], d = ptr[cur + 1] - cs;
                    if (d >= 3) {                                       // b: an arm if it has a read, and is recorded here if a is the smaller anchor
                        if (t >= 1 && cur > a) { arm_end[z] = cur; arm_len[z] = t; arm = true; }
                        break;
                    }
                    if (d != 2 || t == maxt) break;                     // a dead end, or a chain longer than max_arm_reads
                    const uint32_t nx = sg_walk_next(rows, cs, prev);
                    prev = cur; cur = nx; ++t;
                }
            }
        }
    }
    sg_count(&st[BB_ANCHORS], anchor);
    sg_count(&st[BB_ARMS], arm);
}

__global__ void k_bub_pick(const uint32_t *ptr, const int64_t *rows, const int64_t *cols, u64 *st, int r, uint32_t M, const uint32_t *arm_end,
                           const uint32_t *arm_len, uint32_t *removed, uint8_t *flags)
{
    if (!sg_live(st, r)) return;
    const int64_t z = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t n = sg_nnz(st, r);
    bool bubble = false, gone = false;
    if (z < n) {
        const uint32_t b = arm_end[z];
        if (b != BB_NONE) {                                             // k_bub_walk found a = cols[z] < M, an anchor, and an arm of len reads to b
            const uint32_t a = (uint32_t)cols[z], len = arm_len[z];
            const uint32_t ys = ptr[a], ye = ptr[a + 1];
            uint32_t group = 0;
            bool kept = true;
            for (uint32_t y = ys; y < ye; ++y) {
                if (arm_end[y] != b) continue;
                ++group;
                const uint32_t ly = arm_len[y];
                if (ly > len || (ly == len && y < (uint32_t)z)) kept = false;
            }
            bubble = kept && group >= 2;
            gone = !kept;
            if (gone) {                                                 // the walk of k_bub_walk again: it passed len reads of degree 2
                uint32_t prev = a, cur = (uint32_t)rows[z], cnt = 0;
                for (uint32_t i = 0; i < len && cur < M; ++i) {
                    if (atomicExch(&removed[cur], 1u) == 0) { ++cnt; flags[cur] = (uint8_t)(flags[cur] | 8u); }
                    const uint32_t cs = ptr[cur];
                    if (ptr[cur + 1] - cs != 2) break;                  // (never: k_bub_walk went through here on the same tables)
                    const uint32_t nx = sg_walk_next(rows, cs, prev);
                    prev = cur; cur = nx;
                }
                if (cnt) { atomicAdd(&st[BB_READS], (u64)cnt); atomicAdd(sg_removed_slot(st, r), (u64)cnt); }
            }
        }
    }
    sg_count(&st[BB_BUBBLES], bubble);
    sg_count(&st[BB_GONE], gone);
}

}  // namespace

void stage_pop_bubbles(Ctx &c, const elba_bubble_cfg *cfgp)
{
    const elba_bubble_cfg &cfg = sg_enter(c, EV_POP_BUBBLES, cfgp);
    ELBA_REQUIRE(cfg.max_arm_reads >= 1 && cfg.max_arm_reads <= 65535, ELBA_ERR_INVALID_ARG, "pop_bubbles: max_arm_reads outside 1 .. 65535");
    ELBA_REQUIRE(cfg.rounds >= 1 && cfg.rounds <= SG_MAX_ROUNDS, ELBA_ERR_INVALID_ARG, "pop_bubbles: rounds outside 1 .. 64");
    ELBA_REQUIRE(!cfg.reserved[0] && !cfg.reserved[1], ELBA_ERR_INVALID_ARG, "pop_bubbles: reserved words must be 0");
    const int64_t M = c.tr_M, n0 = c.tr_nnz;
    sg_require_32bit(EV_POP_BUBBLES, M < 0xffffffffll && n0 < 0xfffffffell);
    elba_bubble_stats st = sg_stats_begin<elba_bubble_stats>(c);
    st.rounds_run = 1;
    if (M == 0 || n0 == 0) { accepted(c.v, EV_POP_BUBBLES); done(c.v, EV_POP_BUBBLES); c.bb.stats = st; return; }      // no entry: no anchor, the one round removes nothing
    // every buffer of the launch sequence before the first launch
    sg_reserve(c, M, n0);
    c.bb.end.reserve((size_t)(n0 + 1) * 4); c.bb.len.reserve((size_t)(n0 + 1) * 4);
    const SgCall w(c);
    uint32_t *arm_end = c.bb.end.as<uint32_t>(), *arm_len = c.bb.len.as<uint32_t>();
    accepted(c.v, EV_POP_BUBBLES);                              // as in stage_clip_tips: the contigs go, and S is invalid until the counters are back
    u64 h[SG_ST];
    const int moves = sg_run_rounds(w, cfg.rounds, h, [&](int r, const int64_t *rows, const int64_t *cols) {
        hipLaunchKernelGGL(k_bub_begin, dim3(w.nbB), dim3(BB_THREADS), 0, w.s, cols, w.st, r, (uint32_t)M, w.ptr, arm_end, arm_len);
        hipLaunchKernelGGL(k_bub_walk, dim3(w.nbZ), dim3(BB_THREADS), 0, w.s, w.ptr, rows, cols, w.st, r, (uint32_t)cfg.max_arm_reads, (uint32_t)M, arm_end, arm_len);
        hipLaunchKernelGGL(k_bub_pick, dim3(w.nbZ), dim3(BB_THREADS), 0, w.s, w.ptr, rows, cols, w.st, r, (uint32_t)M, arm_end, arm_len, w.removed, w.flags);
    });
    done(c.v, EV_POP_BUBBLES);
    st.anchors = (int64_t)h[BB_ANCHORS]; st.arms = (int64_t)h[BB_ARMS]; st.bubbles = (int64_t)h[BB_BUBBLES]; st.arms_removed = (int64_t)h[BB_GONE];
    st.reads_removed = (int64_t)h[BB_READS];
    st.rounds_run = moves < cfg.rounds ? moves + 1 : cfg.rounds;
    sg_stats_end(c, st);
    c.bb.stats = st;
}

}  // namespace elba
