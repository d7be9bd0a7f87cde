// stars.hip — resolving three-armed stars of the string graph (elba_resolve_stars): the rule of the reference's asmtools/star_resolution.py,
// which runs on a written-out graph after the program.  A read u of degree 3 whose three neighbours all have degree 2 is dropped with its
// edges by the reference's GenerateContigs: one spurious overlap at u costs three contigs and a lost read where there is one path and a
// stray read.  The arms need not be short (no tip), need not rejoin (no bubble), u has no second anchor opposite it (no bridge) and the
// three scores can tie (no weak overlap).  S alone cannot say which arm is the stray one; the overlap matrix before the reduction can: the
// two true neighbours of u overlap each other — their pair was in R and left as transitive through u — and the stray read overlaps neither.
//
// Input and output: the S that tr.hip leaves on the context (tr_out_*), column-major, both triangles, as for tips.hip; and, read only, the
// symmetrised R of the same reduction (Ctx::tr_ptr / tr_sym: CSR over the reads, 16-byte SymEntry, columns ascending; tr_sym_M reads and
// tr_sym_n entries, recorded by stage_transitive_reduction — with no kept pair tr_ptr is not written and tr_sym_n is 0).  The rule is on the
// columns of S and on membership in R alone: deg(v) = length of column v, its neighbours = the rows of column v (ascending).  One ROUND, on
// tables frozen when it starts:
//   centre     a read u with deg(u) == 3 whose three rows x1 < x2 < x3 each have degree exactly 2
//   pair in R  {x, y} such that row x of tr_sym holds column y (R is symmetric: the shorter of rows x and y is searched)
//   odd arm    e = how many of {x1,x2}, {x1,x3}, {x2,x3} are pairs in R; e == 1: the neighbour in no such pair is the centre's odd arm w;
//              e of 0, 2, 3: the centre is left alone
//   removal    every odd arm goes (flag bit 5): every entry whose row or column is one leaves S, the others keep their values and order
// Everything a round decides is read from tables frozen when it starts (ptr, rows, tr_ptr, tr_sym) and what it writes are sets (removed,
// the flag bit), a word per read that only its own lane writes, and sums: the order in which the lanes run does not show in the result.
//
//   k_star_begin    column pointers of the round's S from its column ids (sg_col_ptrs, nnz read on the device)
//   k_star_mark     one lane per read u: deg == 3, three rows, three degrees; only a centre goes on to the three look-ups, each a binary
//                   search of at most floor(log2(len)) + 1 dependent 4-byte loads (SymEntry::col) in the shorter of the two rows.  It leaves
//                   word[u] = SR_W_CENTRE | e << 1 | slot of the odd arm << 3, and for e == 1 does atomicExch on removed[w]: the winner ORs 32
//                   into flags[w] and sets SR_W_WON in its own word.  Every other lane writes word[u] = 0
//   k_star_sums     SR_SUM_BLOCKS workgroups stride over the reads and add the bits of word up: centres, centres by e, reads removed (the
//                   winners), which also goes to *sg_removed_slot(st, r); a wavefront adds its lanes' sums up by shuffles, a workgroup its four
//                   wavefronts' through 96 bytes of LDS, and does one atomicAdd per counter that is not 0: at most 7 x 128 atomics per
//                   round.  The flat kernel counts nothing: a ballot and one atomic per wavefront there is what bridges.hip and weak.hip
//                   measured at four times the call
//   keep flags, scan, scatter: the compaction of sg_rounds.hpp
// Rounds without host synchronisation, in batches of SG_BATCH: the protocol of sg_rounds.hpp (sg_run_rounds).  The rule's part of it: every
// kernel here returns at once when the round before removed nothing.  removed[] is cleared once per call; a read removed in an earlier round is in no
// column and no row of a later round's S, so it is never named again and never wins twice.
//
// Bounds: ptr has M + 1 elements built from the round's nnz, so every column range lies inside it; a lane reads rows only at the three
// entries of a column of length exactly 3, and tests each row below M before ptr is read at it.  A look-up happens only for x, y < RM, where
// RM = min(M, tr_sym_M) if tr_sym_n > 0 and 0 otherwise (then no pointer of an earlier, larger graph is read: every pair is absent); tr_ptr
// has tr_sym_M + 1 elements and is read at x, x + 1 <= RM; both ends of a row's range are clamped to tr_sym_n before tr_sym is read, at
// indices lo <= mid < hi <= tr_sym_n.  word has M elements, written and read below M; removed (M + 1) and flags (M) are written at a row
// of S that was tested below M.  The compaction's bounds are in sg_rounds.hpp.
// Bytes (algorithmic) per round that runs: 8 per entry (column ids) and 4 x M of pointers written; 8 x M of pointers and 4 x M of words
// written by k_star_mark, per read of degree 3 also 24 of rows and 24 of pointers, per centre 24 of R's pointers and at most
// 3 x (floor(log2(len)) + 1) sectors of tr_sym; 4 x M read by k_star_sums: 8 x nnz + 20 x M and the centres' own.  If something is removed,
// the compaction's as well (sg_rounds.hpp: 52 bytes per entry read, 52 per kept entry written, + 28).
#include "sg_rounds.hpp"

namespace elba {

namespace {

constexpr int SR_THREADS = SG_THREADS;          // threads of every kernel here
constexpr int SR_SUM_BLOCKS = 128;              // workgroups of k_star_sums, each with at most seven atomics on st[]
// st[]: 0 centres, 1 .. 4 centres with e = 0 .. 3, 5 reads removed; the protocol's slots: sg_rounds.hpp
enum { SR_CENTRES = 0, SR_PAIRS0 = 1, SR_READS = 5, SR_COUNTERS = 6 };
static_assert(SR_COUNTERS <= SG_LIVE && SR_PAIRS0 + 3 == SR_READS - 1, "the rule's counters lie in front of the protocol's, in k_star_sums' order");
// word[u]: bit 0 u is a centre, bits 1-2 e, bits 3-4 the slot (0 .. 2) of the odd arm among u's rows, bit 5 this lane's exchange on removed[] won
enum : uint32_t { SR_W_CENTRE = 1u, SR_W_E_SHIFT = 1, SR_W_SLOT_SHIFT = 3, SR_W_WON = 32u };

// is {x, y} a pair in R: column y in row x of the symmetrised R, or column x in row y, whichever row is shorter.  RM reads, Rn entries
__device__ __forceinline__ bool sr_pair_in_R(const uint32_t *rptr, const SymEntry *sym, uint32_t RM, uint32_t Rn, uint32_t x, uint32_t y)
{
    if (x >= RM || y >= RM) return false;
    uint32_t a0 = rptr[x], a1 = rptr[x + 1], b0 = rptr[y], b1 = rptr[y + 1];
    if (a1 > Rn) a1 = Rn;
    if (b1 > Rn) b1 = Rn;
    if (a0 > a1) a0 = a1;
    if (b0 > b1) b0 = b1;
    uint32_t lo = a0, hi = a1, key = y;
    if (b1 - b0 < a1 - a0) { lo = b0; hi = b1; key = x; }
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1), col = sym[mid].col;
        if (col == key) return true;
        if (col < key) lo = mid + 1; else hi = mid;
    }
    return false;
}

__global__ void k_star_begin(const int64_t *cols, const u64 *st, int r, uint32_t M, uint32_t *ptr)
{
    if (!sg_live(st, r)) return;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    sg_col_ptrs(cols, sg_nnz(st, r), M, i, ptr);
}

__global__ void k_star_mark(const uint32_t *ptr, const int64_t *rows, const u64 *st, int r, uint32_t M, const uint32_t *rptr, const SymEntry *sym, uint32_t RM,
                            uint32_t Rn, uint32_t *word, uint32_t *removed, uint8_t *flags)
{
    if (!sg_live(st, r)) return;
    const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= M) return;
    uint32_t w = 0;
    const uint32_t s = ptr[u];
    if (ptr[u + 1] - s == 3) {
        const int64_t r0 = rows[s], r1 = rows[s + 1], r2 = rows[s + 2];
        if (r0 >= 0 && r0 < (int64_t)M && r1 >= 0 && r1 < (int64_t)M && r2 >= 0 && r2 < (int64_t)M) {
            const uint32_t x[3] = {(uint32_t)r0, (uint32_t)r1, (uint32_t)r2};
            if (ptr[x[0] + 1] - ptr[x[0]] == 2 && ptr[x[1] + 1] - ptr[x[1]] == 2 && ptr[x[2] + 1] - ptr[x[2]] == 2) {
                const bool p01 = sr_pair_in_R(rptr, sym, RM, Rn, x[0], x[1]), p02 = sr_pair_in_R(rptr, sym, RM, Rn, x[0], x[2]),
                           p12 = sr_pair_in_R(rptr, sym, RM, Rn, x[1], x[2]);
                const uint32_t e = (uint32_t)p01 + (uint32_t)p02 + (uint32_t)p12;
                w = SR_W_CENTRE | e << SR_W_E_SHIFT;
                if (e == 1) {
                    const uint32_t slot = p01 ? 2u : p02 ? 1u : 0u;     // the neighbour in no pair
                    w |= slot << SR_W_SLOT_SHIFT;
                    const uint32_t odd = x[slot];
                    if (atomicExch(&removed[odd], 1u) == 0) { flags[odd] = (uint8_t)(flags[odd] | 32u); w |= SR_W_WON; }
                }
            }
        }
    }
    word[u] = w;
}

// the counts, behind k_star_mark: the bits of word summed over the reads; the removed reads of the round also go where the protocol looks
// for "round r removed something"
__global__ __launch_bounds__(SR_THREADS) void k_star_sums(const uint32_t *word, uint32_t M, u64 *st, int r)
{
    if (!sg_live(st, r)) return;
    uint32_t centres = 0, by_e[4] = {0, 0, 0, 0}, reads = 0;
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < M; i += stride) {
        const uint32_t w = word[i];
        if (w & SR_W_CENTRE) {
            ++centres;
            const uint32_t e = (w >> SR_W_E_SHIFT) & 3u;
            by_e[0] += e == 0; by_e[1] += e == 1; by_e[2] += e == 2; by_e[3] += e == 3;
            reads += (w & SR_W_WON) != 0;
        }
        if (i + stride < i) break;                                      // (M near 2^32: no wrap)
    }
    // six sums per wavefront by shuffles, then per workgroup through LDS: lane k of the first wavefront adds counter k of the four
    // wavefronts up and does the workgroup's one atomicAdd on it, if it is not 0
    __shared__ uint32_t part[SR_THREADS / 64][SR_COUNTERS];
    uint32_t mine[SR_COUNTERS] = {centres, by_e[0], by_e[1], by_e[2], by_e[3], reads};
#pragma unroll
    for (int k = 0; k < SR_COUNTERS; ++k) {
        const uint32_t v = sg_wave_sum(mine[k]);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < SR_COUNTERS) {
        uint32_t v = 0;
#pragma unroll
        for (int w = 0; w < SR_THREADS / 64; ++w) v += part[w][threadIdx.x];
        if (v) {
            atomicAdd(&st[threadIdx.x], (u64)v);                        // (the counters are st[0 .. SR_COUNTERS) in this order)
            if (threadIdx.x == SR_READS) atomicAdd(sg_removed_slot(st, r), (u64)v);
        }
    }
}

}  // namespace

void stage_resolve_stars(Ctx &c, const elba_star_cfg *cfgp)
{
    const elba_star_cfg &cfg = sg_enter(c, EV_RESOLVE_STARS, cfgp);
    ELBA_REQUIRE(cfg.rounds >= 1 && cfg.rounds <= SG_MAX_ROUNDS, ELBA_ERR_INVALID_ARG, "resolve_stars: rounds outside 1 .. 64");
    ELBA_REQUIRE(!cfg.reserved[0] && !cfg.reserved[1] && !cfg.reserved[2], ELBA_ERR_INVALID_ARG, "resolve_stars: reserved words must be 0");
    const int64_t M = c.tr_M, n0 = c.tr_nnz;
    sg_require_32bit(EV_RESOLVE_STARS, M < 0xffffffffll && n0 < 0xfffffffell && c.tr_sym_n < 0xffffffffll);
    elba_star_stats st = sg_stats_begin<elba_star_stats>(c);
    st.rounds_run = 1;
    if (M == 0 || n0 == 0) { accepted(c.v, EV_RESOLVE_STARS); done(c.v, EV_RESOLVE_STARS); c.sr.stats = st; return; }      // no entry: no centre, the one round removes nothing
    // every buffer of the launch sequence before the first launch
    sg_reserve(c, M, n0);
    c.sr.word.reserve((size_t)(M + 1) * 4);
    const SgCall w(c);
    uint32_t *word = c.sr.word.as<uint32_t>();
    // R as the reduction that made this S recorded it; without a kept pair tr_ptr holds nothing of this graph, and no read is looked up
    const uint32_t Rn = (uint32_t)c.tr_sym_n, RM = c.tr_sym_n > 0 ? (uint32_t)(c.tr_sym_M < M ? c.tr_sym_M : M) : 0u;
    const uint32_t *rptr = c.tr_ptr.as<uint32_t>();
    const SymEntry *sym = c.tr_sym.as<SymEntry>();
    accepted(c.v, EV_RESOLVE_STARS);                            // as in stage_clip_tips: the contigs go, and S is invalid until the counters are back
    u64 h[SG_ST];
    const int moves = sg_run_rounds(w, cfg.rounds, h, [&](int r, const int64_t *rows, const int64_t *cols) {
        hipLaunchKernelGGL(k_star_begin, dim3(w.nbB), dim3(SR_THREADS), 0, w.s, cols, w.st, r, (uint32_t)M, w.ptr);
        hipLaunchKernelGGL(k_star_mark, dim3(w.nbM), dim3(SR_THREADS), 0, w.s, w.ptr, rows, w.st, r, (uint32_t)M, rptr, sym, RM, Rn, word, w.removed, w.flags);
        hipLaunchKernelGGL(k_star_sums, dim3(w.nbM < (unsigned)SR_SUM_BLOCKS ? w.nbM : (unsigned)SR_SUM_BLOCKS), dim3(SR_THREADS), 0, w.s, word, (uint32_t)M, w.st, r);
    });
    done(c.v, EV_RESOLVE_STARS);
    st.centres = (int64_t)h[SR_CENTRES]; st.pairs0 = (int64_t)h[SR_PAIRS0]; st.pairs1 = (int64_t)h[SR_PAIRS0 + 1]; st.pairs2 = (int64_t)h[SR_PAIRS0 + 2];
    st.pairs3 = (int64_t)h[SR_PAIRS0 + 3]; st.reads_removed = (int64_t)h[SR_READS];
    st.rounds_run = moves < cfg.rounds ? moves + 1 : cfg.rounds;
    sg_stats_end(c, st);
    c.sr.stats = st;
}

}  // namespace elba
