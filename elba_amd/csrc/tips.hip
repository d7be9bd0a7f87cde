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
//   k_tip_keep      keep[z] = neither row nor column of entry z is removed (0 behind the round's nnz)
//   scan            exclusive, over nnz0 + 1 flags (prims.hip)
//   k_tip_scatter   rows and cols: one lane per entry, 8-byte accesses.  Values (36 bytes = 9 dwords): one lane per DWORD of a 256-entry
//                   tile, so that a wavefront's loads are 256 contiguous bytes and its stores contiguous over every run of kept entries
//                   (one lane per entry would read 36-byte strided records: 9 instructions that each touch 64 x 36 bytes for 256 useful)
//
// Rounds without host synchronisation: the host queues the rounds in batches of TP_BATCH, all sized by the nnz the call starts with;
// st[TP_LIVE + r] (reads the round before removed; 1 for the first) and st[TP_NNZ + r] live on the device, every kernel of a round returns at
// once when the round before removed nothing, and the compaction of a round that removed nothing is skipped too, so S moves between its two
// buffers exactly once per round that removed something.  One synchronisation per batch reads the counters: for rounds <= TP_BATCH, and for
// every graph that is finished within TP_BATCH rounds, that is one per call; the host goes on with the next batch only if every round of this
// one removed something (prims.hip's scan takes its size from the host and cannot return early: a dead round still costs its three launches
// over 4 bytes x nnz0, so at most TP_BATCH - 1 dead rounds are queued whatever `rounds` is).  An odd number of moves swaps the buffers.
//
// Bounds: every index into rows / cols / vals is below the round's nnz (z < n tested, ptr built from n), every read index below M (rows
// and cols of S are; a walk also tests cur < M), a walk reads rows only from a column of length 1 or 2, pos has nnz0 + 1 elements and is
// read at z + 1 <= n <= nnz0, output positions are below the kept count <= nnz0, st slots TP_LIVE + r + 1 <= 72, TP_NNZ + r + 1 <= 144.
// Bytes (algorithmic) per round that removes something: 52 bytes per entry read, 52 per kept entry written, + 4 (keep) + 8 (scan) + the
// 16 bytes per entry the keep kernel reads again; M x 16 for pointers, ntips, anchors.
#include "common.hpp"

namespace elba {

namespace {

constexpr uint32_t TP_NONE = 0xffffffffu;
constexpr int TP_THREADS = 256;                 // threads of every kernel here
constexpr int TP_TILE = 256;                    // entries of S one workgroup of k_tip_scatter moves
constexpr int TP_VWORDS = (int)(sizeof(elba_overlap_t) / 4);
static_assert(sizeof(elba_overlap_t) == 36 && TP_VWORDS == 9, "k_tip_scatter moves the values as 9 dwords");
// st[]: 0 dead ends (first round), 1 tips, 2 reads removed, 3 spared anchors; TP_LIVE + r: the round before r removed that many reads
// (r = 0: 1); TP_NNZ + r: nnz(S) as round r finds it
enum { TP_DEAD = 0, TP_TIPS = 1, TP_READS = 2, TP_SPARED = 3, TP_LIVE = 8, TP_NNZ = 80, TP_ST = 160 };
constexpr int TP_MAX_ROUNDS = 64;
constexpr int TP_BATCH = 4;                     // rounds queued between two looks at the counters
static_assert(TP_LIVE + TP_MAX_ROUNDS + 1 <= TP_NNZ && TP_NNZ + TP_MAX_ROUNDS + 1 <= TP_ST, "one slot per round and one behind the last");

using u64 = unsigned long long;

__global__ void k_tip_init(u64 *st, u64 nnz)
{
    st[TP_LIVE] = 1; st[TP_NNZ] = nnz;
}

__global__ void k_tip_begin(const int64_t *cols, const u64 *st, int r, uint32_t M, uint32_t *ptr, uint32_t *ntips, uint32_t *anchor)
{
    if (st[TP_LIVE + r] == 0) return;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (int64_t)M) { ntips[i] = 0; anchor[i] = TP_NONE; }
    const int64_t n = (int64_t)st[TP_NNZ + r];
    if (i > n) return;
    const int64_t prev = i == 0 ? -1 : cols[i - 1];
    int64_t cur = i == n ? (int64_t)M : cols[i];
    if (cur > (int64_t)M) cur = M;
    for (int64_t k = prev + 1; k <= cur; ++k) ptr[k] = (uint32_t)i;
}

__global__ void k_tip_walk(const uint32_t *ptr, const int64_t *rows, u64 *st, int r, uint32_t maxt, uint32_t M, uint32_t *ntips, uint32_t *anchor)
{
    if (st[TP_LIVE + r] == 0) return;
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
                const uint32_t a = (uint32_t)rows[cs];
                const uint32_t nx = a != prev ? a : (uint32_t)rows[cs + 1];
                prev = cur; cur = nx; ++t;
            }
        }
    }
    const u64 bd = __ballot(dead && r == 0), bt = __ballot(tip);
    const unsigned lane = threadIdx.x & 63;
    if (bd && lane == (unsigned)__builtin_ctzll(bd)) atomicAdd(&st[TP_DEAD], (u64)__builtin_popcountll(bd));
    if (bt && lane == (unsigned)__builtin_ctzll(bt)) atomicAdd(&st[TP_TIPS], (u64)__builtin_popcountll(bt));
}

__global__ void k_tip_mark(const uint32_t *ptr, const int64_t *rows, u64 *st, int r, uint32_t M, const uint32_t *ntips, const uint32_t *anchor,
                           uint32_t *removed, uint8_t *flags)
{
    if (st[TP_LIVE + r] == 0) return;
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
                const uint32_t a = (uint32_t)rows[cs];
                const uint32_t nx = (ptr[cur + 1] - cs == 1 || a != prev) ? a : (uint32_t)rows[cs + 1];
                prev = cur; cur = nx;
            }
            if (cnt) { atomicAdd(&st[TP_READS], (u64)cnt); atomicAdd(&st[TP_LIVE + r + 1], (u64)cnt); }
        }
    }
    const u64 bs = __ballot(spared);
    if (bs && (threadIdx.x & 63) == (unsigned)__builtin_ctzll(bs)) atomicAdd(&st[TP_SPARED], (u64)__builtin_popcountll(bs));
}

__global__ void k_tip_keep(const int64_t *rows, const int64_t *cols, const uint32_t *removed, const u64 *st, int r, int64_t n0, uint32_t *keep)
{
    if (st[TP_LIVE + r] == 0 || st[TP_LIVE + r + 1] == 0) return;       // no round, or a round that removed nothing: S stays where it is
    const int64_t z = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (z > n0) return;
    const int64_t n = (int64_t)st[TP_NNZ + r];
    keep[z] = (z < n && !removed[rows[z]] && !removed[cols[z]]) ? 1u : 0u;
}

__global__ __launch_bounds__(TP_THREADS) void k_tip_scatter(const int64_t *rows, const int64_t *cols, const uint32_t *vals, const uint32_t *pos, u64 *st, int r,
                                                            int64_t n0, int64_t *orows, int64_t *ocols, uint32_t *ovals)
{
    if (st[TP_LIVE + r] == 0 || st[TP_LIVE + r + 1] == 0) return;
    const int64_t n = (int64_t)st[TP_NNZ + r];
    if (blockIdx.x == 0 && threadIdx.x == 0) st[TP_NNZ + r + 1] = pos[n0];     // keep is 0 from n on: the kept count
    const int64_t z0 = (int64_t)blockIdx.x * TP_TILE;
    if (z0 >= n) return;
    const int64_t z = z0 + threadIdx.x;
    if (z < n) {
        const uint32_t p = pos[z];
        if (pos[z + 1] != p) { orows[p] = rows[z]; ocols[p] = cols[z]; }
    }
    const int nw = (int)((n - z0 < TP_TILE ? n - z0 : TP_TILE) * TP_VWORDS);
    const uint32_t *in = vals + z0 * TP_VWORDS;
    uint32_t w[TP_VWORDS];
#pragma unroll
    for (int i = 0; i < TP_VWORDS; ++i) {
        const int g = i * TP_THREADS + (int)threadIdx.x;
        w[i] = g < nw ? in[g] : 0u;
    }
#pragma unroll
    for (int i = 0; i < TP_VWORDS; ++i) {
        const int g = i * TP_THREADS + (int)threadIdx.x;
        if (g >= nw) continue;
        const int e = g / TP_VWORDS, k = g - e * TP_VWORDS;
        const uint32_t p = pos[z0 + e];
        if (pos[z0 + e + 1] != p) ovals[(int64_t)p * TP_VWORDS + k] = w[i];
    }
}

}  // namespace

void stage_clip_tips(Ctx &c, const elba_tip_cfg *cfgp)
{
    enter(c.v, EV_CLIP_TIPS);
    ELBA_REQUIRE(has(c.v, P_S), ELBA_ERR_STATE, "clip_tips: no string graph (call elba_transitive_reduction)");
    ELBA_REQUIRE(cfgp, ELBA_ERR_INVALID_ARG, "clip_tips: null cfg");
    const elba_tip_cfg &cfg = *cfgp;
    ELBA_REQUIRE(cfg.max_tip_reads >= 1 && cfg.max_tip_reads <= 65535, ELBA_ERR_INVALID_ARG, "clip_tips: max_tip_reads outside 1 .. 65535");
    ELBA_REQUIRE(cfg.rounds >= 1 && cfg.rounds <= TP_MAX_ROUNDS, ELBA_ERR_INVALID_ARG, "clip_tips: rounds outside 1 .. 64");
    ELBA_REQUIRE(!cfg.reserved[0] && !cfg.reserved[1], ELBA_ERR_INVALID_ARG, "clip_tips: reserved words must be 0");
    const int64_t M = c.tr_M, n0 = c.tr_nnz;
    ELBA_REQUIRE(M < 0xffffffffll && n0 < 0xfffffffell, ELBA_ERR_UNSUPPORTED, "clip_tips: index ranges beyond 32 bit");
    elba_tip_stats st{};
    st.nreads = M; st.nnz_before = n0; st.nnz_after = n0; st.rounds_run = 1;
    if (M == 0 || n0 == 0) { accepted(c.v, EV_CLIP_TIPS); done(c.v, EV_CLIP_TIPS); c.tpstats = st; return; }      // no entry: no dead end, the one round removes nothing
    hipStream_t s = c.stream;
    // every buffer of the launch sequence before the first launch
    c.tp_ptr.reserve((size_t)(M + 2) * 4); c.tp_ntips.reserve((size_t)(M + 1) * 4); c.tp_anchor.reserve((size_t)(M + 1) * 4); c.tp_removed.reserve((size_t)(M + 1) * 4);
    c.tp_keep.reserve((size_t)(n0 + 2) * 4); c.tp_pos.reserve((size_t)(n0 + 2) * 4); c.tp_st.reserve(TP_ST * 8);
    c.tp_rows.reserve((size_t)(n0 + 1) * 8); c.tp_cols.reserve((size_t)(n0 + 1) * 8); c.tp_vals.reserve((size_t)(n0 + 1) * sizeof(elba_overlap_t));
    c.ws_scan.reserve((size_t)((n0 + 1) / 1024 + 64) * 8);      // (exclusive_scan_u32 sizes it itself; reserved here so that no launch waits for a hipMalloc)
    uint32_t *ptr = c.tp_ptr.as<uint32_t>(), *ntips = c.tp_ntips.as<uint32_t>(), *anchor = c.tp_anchor.as<uint32_t>(), *removed = c.tp_removed.as<uint32_t>();
    uint32_t *keep = c.tp_keep.as<uint32_t>(), *pos = c.tp_pos.as<uint32_t>();
    u64 *dst = c.tp_st.as<u64>();
    int64_t *rows[2] = {c.tr_out_rows.as<int64_t>(), c.tp_rows.as<int64_t>()}, *cols[2] = {c.tr_out_cols.as<int64_t>(), c.tp_cols.as<int64_t>()};
    uint32_t *vals[2] = {c.tr_out_vals.as<uint32_t>(), c.tp_vals.as<uint32_t>()};
    const int64_t lanes = M > n0 + 1 ? M : n0 + 1;
    const unsigned nbB = (unsigned)((lanes + TP_THREADS - 1) / TP_THREADS), nbM = (unsigned)((M + TP_THREADS - 1) / TP_THREADS);
    const unsigned nbK = (unsigned)((n0 + 1 + TP_THREADS - 1) / TP_THREADS), nbS = (unsigned)((n0 + TP_TILE - 1) / TP_TILE);
    accepted(c.v, EV_CLIP_TIPS);                                // S changes under the contigs of the old one, and is itself invalid until the counters are back:
                                                                // a call that fails below leaves no S rather than one in the wrong buffer
    c.tp_t_total.start(s);
    ELBA_HIP(hipMemsetAsync(dst, 0, TP_ST * 8, s));
    ELBA_HIP(hipMemsetAsync(removed, 0, (size_t)(M + 1) * 4, s));
    ELBA_HIP(hipMemsetAsync(keep, 0, (size_t)(n0 + 2) * 4, s));
    hipLaunchKernelGGL(k_tip_init, dim3(1), dim3(1), 0, s, dst, (u64)n0);
    u64 h[TP_ST] = {0};
    int moves = 0, queued = 0;                                  // moves: rounds that removed something, a prefix of the rounds
    while (queued < cfg.rounds) {
        const int end = queued + TP_BATCH < cfg.rounds ? queued + TP_BATCH : cfg.rounds;
        for (int r = queued; r < end; ++r) {
            const int a = r & 1, b = a ^ 1;
            hipLaunchKernelGGL(k_tip_begin, dim3(nbB), dim3(TP_THREADS), 0, s, cols[a], dst, r, (uint32_t)M, ptr, ntips, anchor);
            hipLaunchKernelGGL(k_tip_walk, dim3(nbM), dim3(TP_THREADS), 0, s, ptr, rows[a], dst, r, (uint32_t)cfg.max_tip_reads, (uint32_t)M, ntips, anchor);
            hipLaunchKernelGGL(k_tip_mark, dim3(nbM), dim3(TP_THREADS), 0, s, ptr, rows[a], dst, r, (uint32_t)M, ntips, anchor, removed, c.tr_flags.as<uint8_t>());
            if (r == 0) c.tp_t_compact.start(s);
            hipLaunchKernelGGL(k_tip_keep, dim3(nbK), dim3(TP_THREADS), 0, s, rows[a], cols[a], removed, dst, r, n0, keep);
            exclusive_scan_u32(s, keep, pos, n0 + 1, c.ws_scan);
            hipLaunchKernelGGL(k_tip_scatter, dim3(nbS), dim3(TP_THREADS), 0, s, rows[a], cols[a], vals[a], pos, dst, r, n0, rows[b], cols[b], vals[b]);
            if (r == 0) c.tp_t_compact.stop(s);
        }
        ELBA_HIP(hipGetLastError());
        queued = end;
        c.tp_t_total.stop(s);                                   // (recorded again behind every batch: the last record counts)
        ELBA_HIP(hipMemcpyAsync(h, dst, TP_ST * 8, hipMemcpyDeviceToHost, s));
        ELBA_HIP(hipStreamSynchronize(s));
        while (moves < queued && h[TP_LIVE + moves + 1] > 0) ++moves;
        if (moves < queued) break;                              // a round of this batch removed nothing: the rounds behind it would all return at once
    }
    if (moves & 1) { c.tr_out_rows.swap(c.tp_rows); c.tr_out_cols.swap(c.tp_cols); c.tr_out_vals.swap(c.tp_vals); }
    c.tr_nnz = (int64_t)h[TP_NNZ + moves];
    done(c.v, EV_CLIP_TIPS);
    st.nnz_after = c.tr_nnz; st.entries_removed = n0 - c.tr_nnz;
    st.dead_ends = (int64_t)h[TP_DEAD]; st.tips = (int64_t)h[TP_TIPS]; st.reads_removed = (int64_t)h[TP_READS]; st.spared_anchors = (int64_t)h[TP_SPARED];
    st.rounds_run = moves < cfg.rounds ? moves + 1 : cfg.rounds;
    st.ms_total = c.tp_t_total.ms(); st.ms_compact = c.tp_t_compact.ms();
    c.tpstats = st;
}

}  // namespace elba
