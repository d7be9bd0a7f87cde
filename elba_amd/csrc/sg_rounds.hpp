// sg_rounds.hpp — what the five calls that clean the string graph share (tips.hip: elba_clip_tips, bubbles.hip: elba_pop_bubbles, stars.hip:
// elba_resolve_stars, in rounds; weak.hip: elba_cut_weak_overlaps, bridges.hip: elba_cut_bridges, in one pass): the protocol of the rounds,
// the compaction of S, the frame of a stage function and three device helpers.  A call brings its RULE — kernels that, for round r, read the
// round's S, mark what goes and add what they removed to *sg_removed_slot(st, r) — its cfg checks and its counters; everything else is here,
// and only this file knows the protocol's slots of st[], the two buffers of S and when they swap, and how the counters come back.
//
//   sg_col_ptrs     (device function) column pointers of the round's S from its column ids, nnz read on the device
//   k_sg_keep       keep[z] = neither row nor column of entry z is removed (0 behind the round's nnz)
//   scan            exclusive, over nnz0 + 1 flags (prims.hip)
//   k_sg_scatter    rows and cols: one lane per entry, 8-byte accesses.  Values (36 bytes = 9 dwords): one lane per DWORD of a 256-entry
//                   tile, so that a wavefront's loads are 256 contiguous bytes and its stores contiguous over every run of kept entries
//                   (one lane per entry would read 36-byte strided records: 9 instructions that each touch 64 x 36 bytes for 256 useful)
//
// The host side is three pieces: sg_start (timer, clears, k_sg_init), sg_compact (keep flags, scan, scatter of round r) and sg_read_back
// with sg_settle (the counters back, S in the buffer the moves left it in).  sg_run_rounds loops over them in batches; a one-pass call is
// sg_start, its rule, sg_compact of round 0, sg_read_back, sg_settle.  weak.hip removes entries, not reads: it hands sg_compact a keep
// kernel of its own and a kernel between scan and scatter, and starts by itself, because it has no removed reads to clear.
//
// Rounds without host synchronisation: the host queues the rounds in batches of SG_BATCH, all sized by the nnz the call starts with;
// st[SG_LIVE + r] (reads the round before r removed; 1 for the first) and st[SG_NNZ + r] live on the device, every kernel of a round returns
// at once when the round before removed nothing, and the compaction of a round that removed nothing is skipped too, so S moves between its
// two buffers exactly once per round that removed something.  One synchronisation per batch reads the counters: for rounds <= SG_BATCH, and
// for every graph that is finished within SG_BATCH rounds, that is one per call; the host goes on with the next batch only if every round of
// this one removed something (prims.hip's scan takes its size from the host and cannot return early: a dead round still costs its three
// launches over 4 bytes x nnz0, so at most SG_BATCH - 1 dead rounds are queued whatever `rounds` is).  An odd number of moves swaps the
// buffers.  st[0 .. SG_LIVE) are the rule's own counters.
//
// Bounds: every index into rows / cols / vals is below the round's nnz (z < n tested, ptr built from n), pos has nnz0 + 1 elements and is
// read at z + 1 <= n <= nnz0, output positions are below the kept count <= nnz0, st slots SG_LIVE + r + 1 <= 72, SG_NNZ + r + 1 <= 144;
// removed is read at rows and cols of S, which are below M.
// Bytes (algorithmic) of the compaction of a round that removes something: 52 bytes per entry read, 52 per kept entry written, + 4 (keep)
// + 8 (scan) + the 16 bytes per entry the keep kernel reads again.
#pragma once
#include "common.hpp"

namespace elba {

namespace {

constexpr int SG_THREADS = 256;                 // threads of every kernel here
constexpr int SG_TILE = 256;                    // entries of S one workgroup of k_sg_scatter moves
constexpr int SG_VWORDS = (int)(sizeof(elba_overlap_t) / 4);
static_assert(sizeof(elba_overlap_t) == 36 && SG_VWORDS == 9, "k_sg_scatter moves the values as 9 dwords");
// st[]: 0 .. 7 the rule's counters; SG_LIVE + r: the round before r removed that many reads (r = 0: 1); SG_NNZ + r: nnz(S) as round r finds it
enum { SG_LIVE = 8, SG_NNZ = 80, SG_ST = 160 };
constexpr int SG_MAX_ROUNDS = 64;
constexpr int SG_BATCH = 4;                     // rounds queued between two looks at the counters
static_assert(SG_LIVE + SG_MAX_ROUNDS + 1 <= SG_NNZ && SG_NNZ + SG_MAX_ROUNDS + 1 <= SG_ST, "one slot per round and one behind the last");

using u64 = unsigned long long;

__global__ void k_sg_init(u64 *st, u64 nnz)
{
    st[SG_LIVE] = 1; st[SG_NNZ] = nnz;
}

// The protocol's slots, for the kernels of a rule: round r runs only if the round before it removed something; nnz(S) as it finds it; and
// where it adds what it removed itself (reads, or entries: only "none" matters to the protocol)
__device__ __forceinline__ bool sg_live(const u64 *st, int r) { return st[SG_LIVE + r] != 0; }
__device__ __forceinline__ int64_t sg_nnz(const u64 *st, int r) { return (int64_t)st[SG_NNZ + r]; }
__device__ __forceinline__ u64 *sg_removed_slot(u64 *st, int r) { return &st[SG_LIVE + r + 1]; }

// the sum of v over the 64 lanes of a wavefront, in lane 0; every lane must call it
__device__ __forceinline__ uint32_t sg_wave_sum(uint32_t v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;
}

// one atomicAdd per wavefront for a count of lanes; every lane must call it (mine: 0 or 1, an int as __ballot takes it)
__device__ __forceinline__ void sg_count(u64 *slot, int mine)
{
    const u64 b = __ballot(mine);
    if (b && (threadIdx.x & 63) == (unsigned)__builtin_ctzll(b)) atomicAdd(slot, (u64)__builtin_popcountll(b));
}

// one step of a walk through a read of degree 2 whose column starts at cs: the first row that is not the read it came from.  `only`: the
// column has one row, which is taken whatever prev is (the second walk of k_tip_mark starts at its dead end)
__device__ __forceinline__ uint32_t sg_walk_next(const int64_t *rows, uint32_t cs, uint32_t prev, bool only = false)
{
    const uint32_t x = (uint32_t)rows[cs];
    return (only || x != prev) ? x : (uint32_t)rows[cs + 1];
}

// lane i of a grid of at least n + 1 lanes: ptr[k] = i for every column k in (cols[i - 1], cols[i]] (cols[n] taken as M): M + 1 pointers
__device__ __forceinline__ void sg_col_ptrs(const int64_t *cols, int64_t n, uint32_t M, int64_t i, uint32_t *ptr)
{
    if (i > n) return;
    const int64_t prev = i == 0 ? -1 : cols[i - 1];
    int64_t cur = i == n ? (int64_t)M : cols[i];
    if (cur > (int64_t)M) cur = M;
    for (int64_t k = prev + 1; k <= cur; ++k) ptr[k] = (uint32_t)i;
}

__global__ void k_sg_keep(const int64_t *rows, const int64_t *cols, const uint32_t *removed, const u64 *st, int r, int64_t n0, uint32_t *keep)
{
    if (st[SG_LIVE + r] == 0 || st[SG_LIVE + r + 1] == 0) return;       // no round, or a round that removed nothing: S stays where it is
    const int64_t z = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (z > n0) return;
    const int64_t n = (int64_t)st[SG_NNZ + r];
    keep[z] = (z < n && !removed[rows[z]] && !removed[cols[z]]) ? 1u : 0u;
}

__global__ __launch_bounds__(SG_THREADS) void k_sg_scatter(const int64_t *rows, const int64_t *cols, const uint32_t *vals, const uint32_t *pos, u64 *st, int r,
                                                           int64_t n0, int64_t *orows, int64_t *ocols, uint32_t *ovals)
{
    if (st[SG_LIVE + r] == 0 || st[SG_LIVE + r + 1] == 0) return;
    const int64_t n = (int64_t)st[SG_NNZ + r];
    if (blockIdx.x == 0 && threadIdx.x == 0) st[SG_NNZ + r + 1] = pos[n0];     // keep is 0 from n on: the kept count
    const int64_t z0 = (int64_t)blockIdx.x * SG_TILE;
    if (z0 >= n) return;
    const int64_t z = z0 + threadIdx.x;
    if (z < n) {
        const uint32_t p = pos[z];
        if (pos[z + 1] != p) { orows[p] = rows[z]; ocols[p] = cols[z]; }
    }
    const int nw = (int)((n - z0 < SG_TILE ? n - z0 : SG_TILE) * SG_VWORDS);
    const uint32_t *in = vals + z0 * SG_VWORDS;
    uint32_t w[SG_VWORDS];
#pragma unroll
    for (int i = 0; i < SG_VWORDS; ++i) {
        const int g = i * SG_THREADS + (int)threadIdx.x;
        w[i] = g < nw ? in[g] : 0u;
    }
#pragma unroll
    for (int i = 0; i < SG_VWORDS; ++i) {
        const int g = i * SG_THREADS + (int)threadIdx.x;
        if (g >= nw) continue;
        const int e = g / SG_VWORDS, k = g - e * SG_VWORDS;
        const uint32_t p = pos[z0 + e];
        if (pos[z0 + e + 1] != p) ovals[(int64_t)p * SG_VWORDS + k] = w[i];
    }
}

// ---- the frame of a stage function: enter, check, reserve, `accepted`, launch, `done`, stats ------------------------------------------

// enter, and the two checks every cleaning call makes in front of its own: a valid S and a cfg
template <class Cfg>
inline const Cfg &sg_enter(Ctx &c, Event ev, const Cfg *cfgp)
{
    enter(c.v, ev);
    ELBA_REQUIRE(has(c.v, P_S), ELBA_ERR_STATE, std::string(TABLE[ev].name) + ": no string graph (call elba_transitive_reduction)");
    ELBA_REQUIRE(cfgp, ELBA_ERR_INVALID_ARG, std::string(TABLE[ev].name) + ": null cfg");
    return *cfgp;
}

// behind the cfg checks: the rule's own limits on M and nnz (the kernels index with 32 bits)
inline void sg_require_32bit(Event ev, bool fits)
{
    ELBA_REQUIRE(fits, ELBA_ERR_UNSUPPORTED, std::string(TABLE[ev].name) + ": index ranges beyond 32 bit");
}

// the stats of a call as they stand before it removes anything, and what every call reports when the counters are back
template <class Stats>
inline Stats sg_stats_begin(const Ctx &c)
{
    Stats st{};
    st.nreads = c.tr_M; st.nnz_before = c.tr_nnz; st.nnz_after = c.tr_nnz;
    return st;
}

template <class Stats>
inline void sg_stats_end(Ctx &c, Stats &st)
{
    st.nnz_after = c.tr_nnz; st.entries_removed = st.nnz_before - c.tr_nnz;
    st.ms_total = c.sg.t_total.ms(); st.ms_compact = c.sg.t_compact.ms();
}

// The buffers the protocol itself needs, for an S of M reads and n0 entries: column pointers, the removed set, keep flags and their scan,
// the counters, the second buffer of S.  A call reserves these and its rule's own before its first launch, and only then is `accepted`.
inline void sg_reserve(Ctx &c, int64_t M, int64_t n0)
{
    c.sg.ptr.reserve((size_t)(M + 2) * 4); c.sg.removed.reserve((size_t)(M + 1) * 4);
    c.sg.keep.reserve((size_t)(n0 + 2) * 4); c.sg.pos.reserve((size_t)(n0 + 2) * 4); c.sg.st.reserve(SG_ST * 8);
    c.sg.rows.reserve((size_t)(n0 + 1) * 8); c.sg.cols.reserve((size_t)(n0 + 1) * 8); c.sg.vals.reserve((size_t)(n0 + 1) * sizeof(elba_overlap_t));
    c.ws_scan.reserve((size_t)((n0 + 1) / 1024 + 64) * 8);      // (exclusive_scan_u32 sizes it itself; reserved here so that no launch waits for a hipMalloc)
}

inline unsigned sg_blocks(int64_t lanes) { return (unsigned)((lanes + SG_THREADS - 1) / SG_THREADS); }

// What the launches of a call work with, taken once sg_reserve is through: the context's S (M reads, n0 entries, both > 0) in its two
// buffers — [0] is tr_out_*, where S is when the call starts — the protocol's typed pointers, and the grids of SG_THREADS lanes
struct SgCall {
    Ctx &c;
    const int64_t M, n0;
    hipStream_t s;
    uint32_t *ptr, *removed, *keep, *pos;
    u64 *st;
    uint8_t *flags;
    int64_t *rows[2], *cols[2];
    uint32_t *vals[2];
    unsigned nbM, nbZ, nbB;     // one lane per read, per entry, and for a kernel that clears a table per read beside sg_col_ptrs' n0 + 1 lanes
    explicit SgCall(Ctx &cx)
        : c(cx), M(cx.tr_M), n0(cx.tr_nnz), s(cx.stream), ptr(cx.sg.ptr.as<uint32_t>()), removed(cx.sg.removed.as<uint32_t>()), keep(cx.sg.keep.as<uint32_t>()),
          pos(cx.sg.pos.as<uint32_t>()), st(cx.sg.st.as<u64>()), flags(cx.tr_flags.as<uint8_t>()), rows{cx.tr_out_rows.as<int64_t>(), cx.sg.rows.as<int64_t>()},
          cols{cx.tr_out_cols.as<int64_t>(), cx.sg.cols.as<int64_t>()}, vals{cx.tr_out_vals.as<uint32_t>(), cx.sg.vals.as<uint32_t>()}, nbM(sg_blocks(M)),
          nbZ(sg_blocks(n0)), nbB(sg_blocks(M > n0 + 1 ? M : n0 + 1))
    {
    }
};

// ---- the protocol: a start, the compaction of round r, and the counters back ------------------------------------------------------

// The start of a call whose rule removes READS: t_total, the counters, the removed set and the keep flags (k_sg_keep leaves them alone
// in a round that has nothing to do) cleared, round 0 set up.  The caller has reserved the buffers and named its event `accepted`; S is
// not valid from here until sg_settle.
inline void sg_start(const SgCall &w)
{
    w.c.sg.t_total.start(w.s);
    ELBA_HIP(hipMemsetAsync(w.st, 0, SG_ST * 8, w.s));
    ELBA_HIP(hipMemsetAsync(w.removed, 0, (size_t)(w.M + 1) * 4, w.s));
    ELBA_HIP(hipMemsetAsync(w.keep, 0, (size_t)(w.n0 + 2) * 4, w.s));
    hipLaunchKernelGGL(k_sg_init, dim3(1), dim3(1), 0, w.s, w.st, (u64)w.n0);
}

// The compaction of round r, from buffer r & 1 of S into the other; t_compact spans that of round 0.  keep(rows, cols) queues the kernel
// that writes the n0 + 1 keep flags of the round's S, scanned() what the rule has to do between the scan and the scatter.
template <class Keep, class Scanned>
inline void sg_compact(const SgCall &w, int r, Keep keep, Scanned scanned)
{
    const int a = r & 1, b = a ^ 1;
    if (r == 0) w.c.sg.t_compact.start(w.s);
    keep(w.rows[a], w.cols[a]);
    exclusive_scan_u32(w.s, w.keep, w.pos, w.n0 + 1, w.c.ws_scan);
    scanned();
    hipLaunchKernelGGL(k_sg_scatter, dim3((unsigned)((w.n0 + SG_TILE - 1) / SG_TILE)), dim3(SG_THREADS), 0, w.s, w.rows[a], w.cols[a], w.vals[a], w.pos, w.st, r, w.n0,
                       w.rows[b], w.cols[b], w.vals[b]);
    if (r == 0) w.c.sg.t_compact.stop(w.s);
}

// ... of a rule that removes reads: an entry stays if neither its row nor its column is in the removed set
inline void sg_compact(const SgCall &w, int r)
{
    sg_compact(w, r, [&](const int64_t *rows, const int64_t *cols) {
        hipLaunchKernelGGL(k_sg_keep, dim3(sg_blocks(w.n0 + 1)), dim3(SG_THREADS), 0, w.s, rows, cols, w.removed, w.st, r, w.n0, w.keep);
    }, [] {});
}

// The counters back into h: the one host synchronisation of a one-pass call, or of a batch of rounds (t_total is recorded again behind
// every batch: the last record counts).  Returns `moves` counted on over the rounds below `queued` that removed something.
inline int sg_read_back(const SgCall &w, u64 (&h)[SG_ST], int queued, int moves)
{
    ELBA_HIP(hipGetLastError());
    w.c.sg.t_total.stop(w.s);
    ELBA_HIP(hipMemcpyAsync(h, w.st, SG_ST * 8, hipMemcpyDeviceToHost, w.s));
    ELBA_HIP(hipStreamSynchronize(w.s));
    while (moves < queued && h[SG_LIVE + moves + 1] > 0) ++moves;
    return moves;
}

// S is in the buffer `moves` moves left it in: an odd number swaps the two, and tr_nnz is what the last move kept.  `done` is the caller's.
inline void sg_settle(const SgCall &w, const u64 (&h)[SG_ST], int moves)
{
    Ctx &c = w.c;
    if (moves & 1) { c.tr_out_rows.swap(c.sg.rows); c.tr_out_cols.swap(c.sg.cols); c.tr_out_vals.swap(c.sg.vals); }
    c.tr_nnz = (int64_t)h[SG_NNZ + moves];
}

// Runs up to `rounds` >= 1 rounds and leaves the S the last one made in tr_out_* with tr_nnz.  rule(r, rows, cols) queues the rule's
// kernels of round r on the stream, which read the round's S at rows / cols.  h receives the counters as the last synchronisation found
// them.  Returns the moves: the rounds that removed something, a prefix of the rounds.
template <class Rule>
inline int sg_run_rounds(const SgCall &w, int rounds, u64 (&h)[SG_ST], Rule rule)
{
    sg_start(w);
    int moves = 0, queued = 0;
    while (queued < rounds) {
        const int end = queued + SG_BATCH < rounds ? queued + SG_BATCH : rounds;
        for (int r = queued; r < end; ++r) {
            rule(r, w.rows[r & 1], w.cols[r & 1]);
            sg_compact(w, r);
        }
        queued = end;
        moves = sg_read_back(w, h, queued, moves);
        if (moves < queued) break;                              // a round of this batch removed nothing: the rounds behind it would all return at once
    }
    sg_settle(w, h, moves);
    return moves;
}

}  // namespace

}  // namespace elba
