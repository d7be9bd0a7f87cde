// bridges.hip — cutting bridge chains between two paths of the string graph (elba_cut_bridges): the rule of the reference's
// asmtools/bridge_removal.py, taken from one read to a chain of up to max_bridge_reads reads; the reference's GenerateContigs drops every
// read of degree > 2 with its edges, so a chimeric read that joins the middles of two long paths (the letter H) costs four contigs and the
// two end reads.  The chain is no tip (both flanks are long), no bubble (the chains do not rejoin) and no weak overlap (the scores can tie).
//
// Input and output: the S that tr.hip leaves on the context (tr_out_*), column-major, both triangles, as for tips.hip.  The rule is stated on
// columns alone: deg(v) = length of column v, the neighbours of v = the rows of column v (ascending).  ONE pass, on tables frozen when it starts:
//   anchor     a read of degree >= 3
//   chain      the arm of bubbles.hip: for an entry z of a column a that is an anchor, whose row v1 has degree 2, the walk of tips.hip from v1,
//              "came from" = a; from vi of degree 2 it goes on to the first row of column vi that is not v(i-1).  The first read b of degree >= 3
//              ends it: v1 .. vt, 1 <= t <= max_bridge_reads, is a chain from a to b — if b > a (recorded at its smaller anchor; b == a is no
//              chain).  A read of degree 0 or 1 ends it too (no chain), and so does read max_bridge_reads + 1 (too long)
//   flank      for an entry z of a column u of length exactly 3, with row w: the same walk from w, "came from" = u, counting the reads of degree 2
//              it passes; it stops at the first read whose degree is not 2, or when min_flank_reads are counted: then the flank is LONG
//   bridge     a chain from a to b with deg(a) == deg(b) == 3, the two entries of column a other than z both long flanks, column b holding an
//              entry whose row is vt, and the two other entries of column b both long flanks
//   removal    the reads of every bridge go (flag bit 4): every entry whose row or column is one of them leaves S, the others keep their values
//              and their order.  a and b stay
// Everything the pass decides is read from tables frozen when it starts (ptr, then bit 0 of flank, which k_brg_cut only reads) and what it
// writes are sets (removed, the flag bit, bits 1 and 2 of its own flank word) and sums: the order in which the lanes run does not show in
// the result.
//
//   k_brg_begin     column pointers of S from its column ids (sg_col_ptrs), flank[z] = 0
//   k_brg_flank     one lane per entry z; if its column has length exactly 3 the lane walks at most min_flank_reads dependent steps and writes
//                   flank[z] = 1 for a long flank.  A flank is computed once here and not once per chain that asks for it: a lane's work is
//                   bounded by min_flank_reads, and k_brg_cut reads four words
//   k_brg_cut       one lane per entry z; if deg(col) >= 3 and deg(row) == 2 the lane walks at most max_bridge_reads steps; at an anchor b > col
//                   it has a chain and sets bit 1 of flank[z].  If both ends have degree 3 and the four flank words have bit 0 — vt's entry
//                   of column b is found by comparing its three rows with vt — it is a bridge: bit 2 of flank[z], and the lane walks the
//                   chain again, t reads: removed[vi] = 1 (atomicExch: the winner sets flag bit 4)
//   k_brg_sums      BR_SUM_BLOCKS workgroups stride over the entries and the reads: the three bits of flank sum to long_flanks, chains and
//                   bridges, columns of length >= 3 to anchors, removed to reads_removed, which also goes to *sg_removed_slot(st, 0); every wavefront
//                   adds its lanes' sums up by shuffles and does one atomicAdd per counter that is not 0
//   keep flags, scan, scatter: the compaction of sg_rounds.hpp (sg_compact) as its round 0.  After a pass that removed no read k_sg_keep
//                   and k_sg_scatter return at once and S stays in its buffer; otherwise the two buffers of S are swapped
//
// The walks are dependent loads of a few lanes: an entry of a degree-3 column costs up to min_flank_reads steps of two pointers and one or
// two rows each, an entry of an anchor's column with a degree-2 row up to max_bridge_reads such steps, every other entry the two pointers of
// its column (and of its row).  A first version counted anchors, long flanks, chains and bridges with a ballot and one atomicAdd per
// wavefront on a word of st[], as bubbles.hip counts its arms; on the layout graph of DESIGN 4.12 a sixth of the reads are anchors, nearly
// every wavefront had something to count, and the call took 0.44 ms, four times elba_cut_weak_overlaps on the same S (weak.hip met the same
// and says what 10 000 atomics on one word cost).  So the two flat kernels count nothing: they leave bits, and k_brg_sums adds them up with
// at most 5 x 512 atomics (profiles/bridges_notes.md).  One host synchronisation per call.  No LDS.
//
// Bounds: a lane works on an entry z < n0, the nnz of the call; ptr has M + 1 elements built from n0, so every column range lies in [0, n0);
// rows[z] and cols[z] are tested below M before ptr is read at them, and the walks test cur < M again before every step; a walk reads rows
// only from a column of length 2, at its two entries; flank has n0 + 1 elements and is read and written at entries of columns of length
// exactly 3, inside their ranges, and at the lane's own entry; the second walk of k_brg_cut repeats one that finished on the same tables, for
// exactly t steps; removed (M + 1 elements) and flags (M) are written at reads below M; k_brg_sums reads flank below n0, removed below M and
// ptr at i and i + 1 <= M; keep has n0 + 2 elements, pos n0 + 1 and is read at n0; the compaction's bounds are in sg_rounds.hpp.
// Bytes (algorithmic): k_brg_begin 8 per entry read (column ids), 4 written (flank), 4 x M of pointers written; k_brg_flank 16 per entry read
// (row, column id) and the two pointers of its column, and per step of a walk 8 of pointers and 8 or 16 of rows; k_brg_cut 16 per entry read (row,
// column id) and four pointers, the walks and the 24 + 4 x 4 bytes of the two anchors' columns apart (they touch the chains only); k_brg_sums
// 4 per entry and 8 per read: 48 x nnz + 12 x M.  If something is removed the compaction's as well (sg_rounds.hpp: 52 bytes per entry read, 52 per kept entry written, + 28).
#include "sg_rounds.hpp"

namespace elba {

namespace {

constexpr int BR_THREADS = SG_THREADS;          // threads of every kernel here
constexpr int BR_SUM_BLOCKS = 128;              // workgroups of k_brg_sums: 512 wavefronts, each with at most five atomics on st[]
// st[]: 0 anchors, 1 chains, 2 long flanks, 3 bridges, 4 reads removed; the protocol's slots: sg_rounds.hpp
enum { BR_ANCHORS = 0, BR_CHAINS = 1, BR_LONG = 2, BR_BRIDGES = 3, BR_READS = 4 };
static_assert(BR_READS < SG_LIVE, "the rule's counters lie in front of the protocol's");
// flank[z]: bit 0 the flank of entry z is long (k_brg_flank), bit 1 entry z starts a chain, bit 2 that chain is a bridge (k_brg_cut)
enum : uint32_t { BR_F_LONG = 1u, BR_F_CHAIN = 2u, BR_F_BRIDGE = 4u };

__global__ void k_brg_begin(const int64_t *cols, int64_t n, uint32_t M, uint32_t *ptr, uint32_t *flank)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= n) flank[i] = 0;
    sg_col_ptrs(cols, n, M, i, ptr);
}

__global__ void k_brg_flank(const uint32_t *ptr, const int64_t *rows, const int64_t *cols, int64_t n, uint32_t minf, uint32_t M, uint32_t *flank)
{
    const int64_t z = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (z >= n) return;
    const int64_t c64 = cols[z], r64 = rows[z];
    if (c64 < 0 || c64 >= (int64_t)M || r64 < 0 || r64 >= (int64_t)M) return;
    const uint32_t u = (uint32_t)c64;
    if (ptr[u + 1] - ptr[u] != 3) return;
    uint32_t prev = u, cur = (uint32_t)r64, cnt = 0;
    while (cnt < minf && cur < M) {
        const uint32_t cs = ptr[cur];
        if (ptr[cur + 1] - cs != 2) break;                              // the flank ends here: an anchor, a dead end
        ++cnt;
        const uint32_t nx = sg_walk_next(rows, cs, prev);
        prev = cur; cur = nx;
    }
    if (cnt == minf) flank[z] = BR_F_LONG;
}

__global__ void k_brg_cut(const uint32_t *ptr, const int64_t *rows, const int64_t *cols, int64_t n, uint32_t maxt, uint32_t M, uint32_t *flank,
                          uint32_t *removed, uint8_t *flags)
{
    const int64_t z = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (z >= n) return;
    const int64_t c64 = cols[z], r64 = rows[z];
    if (c64 < 0 || c64 >= (int64_t)M || r64 < 0 || r64 >= (int64_t)M) return;
    const uint32_t a = (uint32_t)c64, v1 = (uint32_t)r64;
    const uint32_t as = ptr[a], da = ptr[a + 1] - as;
    if (da < 3 || ptr[v1 + 1] - ptr[v1] != 2) return;
    uint32_t prev = a, cur = v1, t = 0, bs = 0, db = 0;                 // t reads in the chain so far
    bool chain = false;
    while (cur < M) {
        const uint32_t cs = ptr[cur], d = ptr[cur + 1] - cs;
        if (d >= 3) {                                                   // b: a chain (t >= 1 here), recorded if a is the smaller anchor
            if (cur > a) { chain = true; bs = cs; db = d; }
            break;
        }
        if (d != 2 || t == maxt) break;                                 // a dead end, or a chain longer than max_bridge_reads
        const uint32_t nx = sg_walk_next(rows, cs, prev);
        prev = cur; cur = nx; ++t;
    }
    if (!chain) return;
    bool bridge = false;
    if (da == 3 && db == 3) {                                           // prev is vt
        uint32_t longs = 0, mine = 0;
        for (uint32_t y = as; y < as + 3; ++y) if ((int64_t)y != z) longs += flank[y] & BR_F_LONG;
        for (uint32_t y = bs; y < bs + 3; ++y) {
            if (rows[y] == (int64_t)prev) ++mine; else longs += flank[y] & BR_F_LONG;
        }
        bridge = mine == 1 && longs == 4;
    }
    atomicOr(&flank[z], bridge ? BR_F_CHAIN | BR_F_BRIDGE : BR_F_CHAIN);      // (atomic: other lanes read bit 0 of this word meanwhile; it does not change)
    if (bridge) {                                                       // the walk again: it passed t reads of degree 2
        uint32_t p = a, c = v1;
        for (uint32_t i = 0; i < t && c < M; ++i) {
            if (atomicExch(&removed[c], 1u) == 0) flags[c] = (uint8_t)(flags[c] | 16u);
            const uint32_t cs = ptr[c];
            if (ptr[c + 1] - cs != 2) break;                            // (never: the first walk went through here on the same tables)
            const uint32_t nx = sg_walk_next(rows, cs, p);
            p = c; c = nx;
        }
    }
}

// the counts, behind k_brg_cut: BR_SUM_BLOCKS workgroups stride over the n entries (the three bits of flank) and the M reads (degree >= 3,
// removed); every wavefront adds its lanes' sums up by shuffles and does one atomicAdd per counter that is not 0.  The removed reads also go
// where the compaction looks for "round 0 removed something"
__global__ __launch_bounds__(BR_THREADS) void k_brg_sums(const uint32_t *ptr, const uint32_t *flank, const uint32_t *removed, int64_t n, uint32_t M, u64 *st)
{
    uint32_t anchors = 0, chains = 0, longs = 0, bridges = 0, reads = 0;
    const int64_t top = n > (int64_t)M ? n : (int64_t)M, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < top; i += stride) {
        if (i < n) {
            const uint32_t w = flank[i];
            longs += w & 1u; chains += (w >> 1) & 1u; bridges += (w >> 2) & 1u;
        }
        if (i < (int64_t)M) {
            anchors += ptr[i + 1] - ptr[i] >= 3;
            reads += removed[i] != 0;
        }
    }
    anchors = sg_wave_sum(anchors); chains = sg_wave_sum(chains); longs = sg_wave_sum(longs); bridges = sg_wave_sum(bridges); reads = sg_wave_sum(reads);
    if ((threadIdx.x & 63) == 0) {
        if (anchors) atomicAdd(&st[BR_ANCHORS], (u64)anchors);
        if (chains) atomicAdd(&st[BR_CHAINS], (u64)chains);
        if (longs) atomicAdd(&st[BR_LONG], (u64)longs);
        if (bridges) atomicAdd(&st[BR_BRIDGES], (u64)bridges);
        if (reads) { atomicAdd(&st[BR_READS], (u64)reads); atomicAdd(sg_removed_slot(st, 0), (u64)reads); }
    }
}

}  // namespace

void stage_cut_bridges(Ctx &c, const elba_bridge_cfg *cfgp)
{
    const elba_bridge_cfg &cfg = sg_enter(c, EV_CUT_BRIDGES, cfgp);
    ELBA_REQUIRE(cfg.max_bridge_reads >= 1 && cfg.max_bridge_reads <= 65534, ELBA_ERR_INVALID_ARG, "cut_bridges: max_bridge_reads outside 1 .. 65534");
    ELBA_REQUIRE(cfg.min_flank_reads > cfg.max_bridge_reads && cfg.min_flank_reads <= 65535, ELBA_ERR_INVALID_ARG,
                 "cut_bridges: min_flank_reads outside max_bridge_reads + 1 .. 65535");
    ELBA_REQUIRE(!cfg.reserved[0] && !cfg.reserved[1], ELBA_ERR_INVALID_ARG, "cut_bridges: reserved words must be 0");
    const int64_t M = c.tr_M, n0 = c.tr_nnz;
    sg_require_32bit(EV_CUT_BRIDGES, M < 0xffffffffll && n0 < 0xfffffffell);
    elba_bridge_stats st = sg_stats_begin<elba_bridge_stats>(c);
    if (M == 0 || n0 == 0) { accepted(c.v, EV_CUT_BRIDGES); done(c.v, EV_CUT_BRIDGES); c.br.stats = st; return; }      // no entry: no anchor
    // every buffer of the launch sequence before the first launch
    sg_reserve(c, M, n0);
    c.br.flank.reserve((size_t)(n0 + 1) * 4);
    const SgCall w(c);
    uint32_t *flank = c.br.flank.as<uint32_t>();
    const int64_t *rows = w.rows[0], *cols = w.cols[0];
    accepted(c.v, EV_CUT_BRIDGES);                              // as in stage_clip_tips: the contigs go, and S is invalid until the counters are back
    sg_start(w);
    hipLaunchKernelGGL(k_brg_begin, dim3(w.nbB), dim3(BR_THREADS), 0, w.s, cols, n0, (uint32_t)M, w.ptr, flank);
    hipLaunchKernelGGL(k_brg_flank, dim3(w.nbZ), dim3(BR_THREADS), 0, w.s, w.ptr, rows, cols, n0, (uint32_t)cfg.min_flank_reads, (uint32_t)M, flank);
    hipLaunchKernelGGL(k_brg_cut, dim3(w.nbZ), dim3(BR_THREADS), 0, w.s, w.ptr, rows, cols, n0, (uint32_t)cfg.max_bridge_reads, (uint32_t)M, flank, w.removed, w.flags);
    hipLaunchKernelGGL(k_brg_sums, dim3(w.nbB < (unsigned)BR_SUM_BLOCKS ? w.nbB : (unsigned)BR_SUM_BLOCKS), dim3(BR_THREADS), 0, w.s, w.ptr, flank, w.removed, n0, (uint32_t)M, w.st);
    sg_compact(w, 0);
    u64 h[SG_ST];
    sg_settle(w, h, sg_read_back(w, h, 1, 0));
    done(c.v, EV_CUT_BRIDGES);
    st.anchors = (int64_t)h[BR_ANCHORS]; st.chains = (int64_t)h[BR_CHAINS]; st.long_flanks = (int64_t)h[BR_LONG]; st.bridges = (int64_t)h[BR_BRIDGES];
    st.reads_removed = (int64_t)h[BR_READS];
    sg_stats_end(c, st);
    c.br.stats = st;
}

}  // namespace elba
