// weak.hip — cutting weak overlaps at branching read ends of the string graph (elba_cut_weak_overlaps): not in the reference, whose
// GenerateContigs drops every read of degree > 2 with its edges.  Where an end of a read has its true overlap and a much weaker one (a repeat
// copy, a chance alignment) that leads into a long path, the branch is neither a tip nor a bubble; this call removes the weaker ENTRY, no read.
//
// Input and output: the S that tr.hip leaves on the context (tr_out_*), column-major, both triangles, as for tips.hip.  The rule is stated on
// the columns of S and on two fields of an entry z of column c with row r: side(z) = direction & 1 (the end of read c the overlap lies on) and
// weight(z) = score.  ONE pass, on tables frozen when it starts:
//   cnt, best   cnt(c, e) = entries of column c with side e, best(c, e) = their largest score
//   weak        z is weak at its column when cnt(c, side) >= 2, best(c, side) > 0 and (int64)score * 65536 < (int64)min_ratio_q16 * best
//   removed     z is weak at its column, or its mirror image — the entry of column r whose row is c, if S holds one — is weak at column r
//   survivors   keep their values and their order.  No read is removed, the read flags are not touched
// What the pass decides is read from tables that are complete before anything reads them (best, cnt), and what it writes are flags, integer
// maxima and sums: the order in which the lanes run does not show in the result.
//
//   k_weak_begin    column pointers of S from its column ids (sg_col_ptrs), best = INT32_MIN, cnt = nweak = after = 0 for the 2 M sides
//   k_weak_fold     one lane per entry: atomicMax of its score into best[2 c + side], atomicAdd 1 into cnt[2 c + side]
//   k_weak_keep     one lane per entry: weak at its own column from best / cnt; the mirror image by binary search for c in the rows of
//                   column r (ascending), and whether THAT is weak at column r, from its own score and side: no per-entry weak array is
//                   stored.  keep[z] = neither; a weak entry adds 1 to nweak[2 c + side], a kept one 1 to after[2 c + side].  It stands
//                   beside k_sg_keep of sg_rounds.hpp, which asks the removed READS instead
//   scan, k_weak_removed, k_sg_scatter: the compaction of sg_rounds.hpp (sg_compact), as its round 0.  One lane takes the removed-entry
//                   count from the scan (n - pos[n]) into the protocol's slot for what round 0 removed, so the scatter of a pass that
//                   removed nothing returns at once and S stays in its buffer; otherwise the two buffers of S are swapped
//   k_weak_sides    WK_SIDE_BLOCKS workgroups stride over the 2 M sides: cnt >= 2 counts a branch side, cnt >= 1 with after == 0 an emptied
//                   one, nweak sums to the weak entries; every wavefront adds its lanes' sums up by shuffles and does one atomicAdd per
//                   counter that is not 0
//
// Work is linear in nnz whatever a column's length: a lane touches its own entry, three table slots of its column, and log2(deg(r)) rows
// of the mirror's column; sg_col_ptrs writes every pointer once.  The lanes of a hub column all hit the same two words in k_weak_fold; the
// atomics are integer max and add at the L2, order-free, and cheap while their addresses differ: 1.3 M of them take 13 us on the layout
// graph of DESIGN 4.12, so a wavefront-level fold in front of them has nothing to win there.  What is NOT cheap is one atomic per
// wavefront on ONE counter: 10 000 wavefronts adding to the same word took 130 to 220 us, which is why no kernel here counts into st[]
// per wavefront of a flat grid.  One host synchronisation per call.  No LDS.
//
// Bounds: a lane works on an entry z < n0, the nnz of the call; rows[z] and cols[z] are tested below M before any table is read at them;
// ptr has M + 1 elements built from n0, so every column range lies in [0, n0) and the binary search reads rows and vals only there; best,
// cnt, nweak and after have 2 M elements and are indexed at 2 v + (0 | 1) with v < M, or at i < 2 M in k_weak_sides; keep has n0 + 1 flags
// and lane n0 writes the 0 behind the last; pos has n0 + 1 elements and is read at n0; the compaction's bounds are in sg_rounds.hpp.
// Bytes (algorithmic): k_weak_begin 8 per entry read (column ids), 4 (M + 1) + 32 M written; k_weak_fold 8 + 8 per entry read (column id;
// score and direction: two dwords of the 36-byte value) and two atomics; k_weak_keep 16 + 8 per entry (row, column id, score, direction),
// 16 of tables, the mirror's 8 + 16 and the rows of the search, 4 written and one or two atomics; k_weak_sides 24 M.  If something is
// removed the compaction's as well (sg_rounds.hpp: 52 bytes per entry read, 52 per kept entry written, + 8 for the scan).
#include "sg_rounds.hpp"

namespace elba {

namespace {

constexpr int WK_THREADS = SG_THREADS;          // threads of every kernel here
// st[]: 0 branch sides, 1 weak entries, 2 sides emptied; the removed entries and the kept count are in the protocol's slots (sg_rounds.hpp)
enum { WK_BRANCH = 0, WK_WEAK = 1, WK_EMPTIED = 2 };
static_assert(WK_EMPTIED < SG_LIVE, "the rule's counters lie in front of the protocol's");
constexpr int32_t WK_NO_BEST = (int32_t)0x80000000;

constexpr int WK_SIDE_BLOCKS = 128;             // workgroups of k_weak_sides: 512 wavefronts, each with at most three atomics on st[]

__device__ __forceinline__ bool wk_weak(int32_t score, uint32_t cnt, int32_t best, int32_t q16)
{
    return cnt >= 2 && best > 0 && (int64_t)score * 65536 < (int64_t)q16 * (int64_t)best;
}

__global__ void k_weak_begin(const int64_t *cols, int64_t n, uint32_t M, uint32_t *ptr, int32_t *best, uint32_t *cnt, uint32_t *nweak, uint32_t *after)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 2 * (int64_t)M) { best[i] = WK_NO_BEST; cnt[i] = 0; nweak[i] = 0; after[i] = 0; }
    sg_col_ptrs(cols, n, M, i, ptr);
}

__global__ void k_weak_fold(const int64_t *cols, const elba_overlap_t *vals, int64_t n, uint32_t M, int32_t *best, uint32_t *cnt)
{
    const int64_t z = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (z >= n) return;
    const int64_t c = cols[z];
    if (c < 0 || c >= (int64_t)M) return;
    const size_t side = 2 * (size_t)c + (size_t)(vals[z].direction & 1);
    atomicMax(&best[side], vals[z].score);
    atomicAdd(&cnt[side], 1u);
}

__global__ void k_weak_keep(const uint32_t *ptr, const int64_t *rows, const int64_t *cols, const elba_overlap_t *vals, int64_t n, uint32_t M, int32_t q16,
                            const int32_t *best, const uint32_t *cnt, uint32_t *nweak, uint32_t *after, uint32_t *keep)
{
    const int64_t z = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (z > n) return;
    if (z == n) { keep[z] = 0u; return; }                               // the scan runs over n + 1 flags: pos[n] is the kept count
    const int64_t r = rows[z], c = cols[z];
    bool kept = true;
    if (r >= 0 && r < (int64_t)M && c >= 0 && c < (int64_t)M) {
        const size_t side = 2 * (size_t)c + (size_t)(vals[z].direction & 1);
        const bool weak = wk_weak(vals[z].score, cnt[side], best[side], q16);
        bool mirror_weak = false;
        uint32_t lo = ptr[r], hi = ptr[r + 1];                          // column r: rows ascending; the mirror image is its entry with row c
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (rows[mid] < c) lo = mid + 1; else hi = mid;
        }
        if (lo < ptr[r + 1] && rows[lo] == c) {
            const size_t ms = 2 * (size_t)r + (size_t)(vals[lo].direction & 1);
            mirror_weak = wk_weak(vals[lo].score, cnt[ms], best[ms], q16);
        }
        kept = !weak && !mirror_weak;
        if (weak) atomicAdd(&nweak[side], 1u);
        if (kept) atomicAdd(&after[side], 1u);
    }
    keep[z] = kept ? 1u : 0u;
}

// behind the scan: what the pass removed, where k_sg_scatter looks for "round 0 removed something"
__global__ void k_weak_removed(const uint32_t *pos, int64_t n, u64 *st)
{
    *sg_removed_slot(st, 0) = (u64)n - (u64)pos[n];
}

__global__ __launch_bounds__(WK_THREADS) void k_weak_sides(const uint32_t *cnt, const uint32_t *nweak, const uint32_t *after, uint32_t M, u64 *st)
{
    uint32_t branch = 0, emptied = 0, weak = 0;
    const int64_t sides = 2 * (int64_t)M, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < sides; i += stride) {
        const uint32_t k = cnt[i];
        branch += k >= 2;
        emptied += k >= 1 && after[i] == 0;
        weak += nweak[i];
    }
    branch = sg_wave_sum(branch); emptied = sg_wave_sum(emptied); weak = sg_wave_sum(weak);
    if ((threadIdx.x & 63) == 0) {
        if (branch) atomicAdd(&st[WK_BRANCH], (u64)branch);
        if (emptied) atomicAdd(&st[WK_EMPTIED], (u64)emptied);
        if (weak) atomicAdd(&st[WK_WEAK], (u64)weak);
    }
}

}  // namespace

void stage_cut_weak_overlaps(Ctx &c, const elba_weak_cfg *cfgp)
{
    const elba_weak_cfg &cfg = sg_enter(c, EV_CUT_WEAK_OVERLAPS, cfgp);
    ELBA_REQUIRE(cfg.min_ratio_q16 >= 1 && cfg.min_ratio_q16 <= 65536, ELBA_ERR_INVALID_ARG, "cut_weak_overlaps: min_ratio_q16 outside 1 .. 65536");
    ELBA_REQUIRE(!cfg.reserved[0] && !cfg.reserved[1] && !cfg.reserved[2], ELBA_ERR_INVALID_ARG, "cut_weak_overlaps: reserved words must be 0");
    const int64_t M = c.tr_M, n0 = c.tr_nnz;
    sg_require_32bit(EV_CUT_WEAK_OVERLAPS, M < 0x7fffffffll && n0 < 0xfffffffell);         // (2 M sides)
    elba_weak_stats st = sg_stats_begin<elba_weak_stats>(c);
    if (M == 0 || n0 == 0) { accepted(c.v, EV_CUT_WEAK_OVERLAPS); done(c.v, EV_CUT_WEAK_OVERLAPS); c.wk.stats = st; return; }      // no entry: no side has two
    // every buffer of the launch sequence before the first launch
    sg_reserve(c, M, n0);
    c.wk.best.reserve((size_t)(2 * M + 2) * 4); c.wk.cnt.reserve((size_t)(2 * M + 2) * 4); c.wk.nweak.reserve((size_t)(2 * M + 2) * 4);
    c.wk.after.reserve((size_t)(2 * M + 2) * 4);
    const SgCall w(c);
    uint32_t *cnt = c.wk.cnt.as<uint32_t>(), *nweak = c.wk.nweak.as<uint32_t>(), *after = c.wk.after.as<uint32_t>();
    int32_t *best = c.wk.best.as<int32_t>();
    const elba_overlap_t *vals = c.tr_out_vals.as<elba_overlap_t>();
    const unsigned nbB = sg_blocks(2 * M > n0 + 1 ? 2 * M : n0 + 1), nbAll = sg_blocks(2 * M), nbM = nbAll < (unsigned)WK_SIDE_BLOCKS ? nbAll : (unsigned)WK_SIDE_BLOCKS;
    accepted(c.v, EV_CUT_WEAK_OVERLAPS);                        // as in stage_clip_tips: the contigs go, and S is invalid until the counters are back
    // the start is this file's, not sg_start: no read is removed, and k_weak_keep writes all n0 + 1 flags, so neither is cleared
    c.sg.t_total.start(w.s);
    ELBA_HIP(hipMemsetAsync(w.st, 0, SG_ST * 8, w.s));
    hipLaunchKernelGGL(k_sg_init, dim3(1), dim3(1), 0, w.s, w.st, (u64)n0);
    hipLaunchKernelGGL(k_weak_begin, dim3(nbB), dim3(WK_THREADS), 0, w.s, w.cols[0], n0, (uint32_t)M, w.ptr, best, cnt, nweak, after);
    hipLaunchKernelGGL(k_weak_fold, dim3(w.nbZ), dim3(WK_THREADS), 0, w.s, w.cols[0], vals, n0, (uint32_t)M, best, cnt);
    sg_compact(w, 0, [&](const int64_t *rows, const int64_t *cols) {
        hipLaunchKernelGGL(k_weak_keep, dim3(sg_blocks(n0 + 1)), dim3(WK_THREADS), 0, w.s, w.ptr, rows, cols, vals, n0, (uint32_t)M, (int32_t)cfg.min_ratio_q16, best, cnt, nweak, after, w.keep);
    }, [&] { hipLaunchKernelGGL(k_weak_removed, dim3(1), dim3(1), 0, w.s, w.pos, n0, w.st); });
    hipLaunchKernelGGL(k_weak_sides, dim3(nbM), dim3(WK_THREADS), 0, w.s, cnt, nweak, after, (uint32_t)M, w.st);
    u64 h[SG_ST];
    sg_settle(w, h, sg_read_back(w, h, 1, 0));
    done(c.v, EV_CUT_WEAK_OVERLAPS);
    st.branch_sides = (int64_t)h[WK_BRANCH]; st.weak_entries = (int64_t)h[WK_WEAK]; st.sides_emptied = (int64_t)h[WK_EMPTIED];
    sg_stats_end(c, st);                                        // (entries_removed: both images, nnz_before - nnz_after)
    c.wk.stats = st;
}

}  // namespace elba
