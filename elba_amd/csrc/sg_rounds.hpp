// sg_rounds.hpp — what the calls that take reads out of the string graph in rounds share (tips.hip: elba_clip_tips, bubbles.hip:
// elba_pop_bubbles, stars.hip: elba_resolve_stars): the round-batch protocol and the compaction of S.  A call brings its RULE — kernels that, for round r, read the
// round's S and set removed[v] = 1 for every read that goes, adding the reads they removed to st[SG_LIVE + r + 1]; everything else is here.
// weak.hip (elba_cut_weak_overlaps) removes entries, not reads, in one pass: it brings a keep kernel of its own beside k_sg_keep and uses
// sg_col_ptrs, sg_reserve, k_sg_init and k_sg_scatter as round 0 of the protocol, without sg_run_rounds.  bridges.hip (elba_cut_bridges)
// removes reads in one pass and runs round 0 the same way, with k_sg_keep.
//
//   sg_col_ptrs     (device function) column pointers of the round's S from its column ids, nnz read on the device
//   k_sg_keep       keep[z] = neither row nor column of entry z is removed (0 behind the round's nnz)
//   scan            exclusive, over nnz0 + 1 flags (prims.hip)
//   k_sg_scatter    rows and cols: one lane per entry, 8-byte accesses.  Values (36 bytes = 9 dwords): one lane per DWORD of a 256-entry
//                   tile, so that a wavefront's loads are 256 contiguous bytes and its stores contiguous over every run of kept entries
//                   (one lane per entry would read 36-byte strided records: 9 instructions that each touch 64 x 36 bytes for 256 useful)
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

// The buffers the protocol itself needs, for an S of M reads and n0 entries: column pointers, the removed set, keep flags and their scan,
// the counters, the second buffer of S.  A call reserves these and its rule's own before its first launch, and only then is `accepted`.
inline void sg_reserve(Ctx &c, int64_t M, int64_t n0)
{
    c.tp_ptr.reserve((size_t)(M + 2) * 4); c.tp_removed.reserve((size_t)(M + 1) * 4);
    c.tp_keep.reserve((size_t)(n0 + 2) * 4); c.tp_pos.reserve((size_t)(n0 + 2) * 4); c.tp_st.reserve(SG_ST * 8);
    c.tp_rows.reserve((size_t)(n0 + 1) * 8); c.tp_cols.reserve((size_t)(n0 + 1) * 8); c.tp_vals.reserve((size_t)(n0 + 1) * sizeof(elba_overlap_t));
    c.ws_scan.reserve((size_t)((n0 + 1) / 1024 + 64) * 8);      // (exclusive_scan_u32 sizes it itself; reserved here so that no launch waits for a hipMalloc)
}

// Runs up to `rounds` rounds on the context's S (c.tr_M reads, c.tr_nnz entries, both > 0) and leaves the S the last one made in tr_out_*
// with tr_nnz.  rule(r, rows, cols) queues the rule's kernels of round r on c.stream, which read the round's S at rows / cols.  h receives
// the counters as the last synchronisation found them.  Returns the moves: the rounds that removed something, a prefix of the rounds.
// t_total spans the call, t_compact the compaction of the first round.  The caller has reserved the buffers and named its event `accepted`;
// S is not valid while this runs, and `done` is the caller's when it returns.
template <class Rule>
inline int sg_run_rounds(Ctx &c, int rounds, EventTimer &t_total, EventTimer &t_compact, u64 (&h)[SG_ST], Rule rule)
{
    const int64_t M = c.tr_M, n0 = c.tr_nnz;
    hipStream_t s = c.stream;
    uint32_t *removed = c.tp_removed.as<uint32_t>(), *keep = c.tp_keep.as<uint32_t>(), *pos = c.tp_pos.as<uint32_t>();
    u64 *dst = c.tp_st.as<u64>();
    int64_t *rows[2] = {c.tr_out_rows.as<int64_t>(), c.tp_rows.as<int64_t>()}, *cols[2] = {c.tr_out_cols.as<int64_t>(), c.tp_cols.as<int64_t>()};
    uint32_t *vals[2] = {c.tr_out_vals.as<uint32_t>(), c.tp_vals.as<uint32_t>()};
    const unsigned nbK = (unsigned)((n0 + 1 + SG_THREADS - 1) / SG_THREADS), nbS = (unsigned)((n0 + SG_TILE - 1) / SG_TILE);
    t_total.start(s);
    ELBA_HIP(hipMemsetAsync(dst, 0, SG_ST * 8, s));
    ELBA_HIP(hipMemsetAsync(removed, 0, (size_t)(M + 1) * 4, s));
    ELBA_HIP(hipMemsetAsync(keep, 0, (size_t)(n0 + 2) * 4, s));
    hipLaunchKernelGGL(k_sg_init, dim3(1), dim3(1), 0, s, dst, (u64)n0);
    for (int i = 0; i < SG_ST; ++i) h[i] = 0;
    int moves = 0, queued = 0;
    while (queued < rounds) {
        const int end = queued + SG_BATCH < rounds ? queued + SG_BATCH : rounds;
        for (int r = queued; r < end; ++r) {
            const int a = r & 1, b = a ^ 1;
            rule(r, rows[a], cols[a]);
            if (r == 0) t_compact.start(s);
            hipLaunchKernelGGL(k_sg_keep, dim3(nbK), dim3(SG_THREADS), 0, s, rows[a], cols[a], removed, dst, r, n0, keep);
            exclusive_scan_u32(s, keep, pos, n0 + 1, c.ws_scan);
            hipLaunchKernelGGL(k_sg_scatter, dim3(nbS), dim3(SG_THREADS), 0, s, rows[a], cols[a], vals[a], pos, dst, r, n0, rows[b], cols[b], vals[b]);
            if (r == 0) t_compact.stop(s);
        }
        ELBA_HIP(hipGetLastError());
        queued = end;
        t_total.stop(s);                                        // (recorded again behind every batch: the last record counts)
        ELBA_HIP(hipMemcpyAsync(h, dst, SG_ST * 8, hipMemcpyDeviceToHost, s));
        ELBA_HIP(hipStreamSynchronize(s));
        while (moves < queued && h[SG_LIVE + moves + 1] > 0) ++moves;
        if (moves < queued) break;                              // a round of this batch removed nothing: the rounds behind it would all return at once
    }
    if (moves & 1) { c.tr_out_rows.swap(c.tp_rows); c.tr_out_cols.swap(c.tp_cols); c.tr_out_vals.swap(c.tp_vals); }
    c.tr_nnz = (int64_t)h[SG_NNZ + moves];
    return moves;
}

}  // namespace

}  // namespace elba
