// components.hip — connected components of the string graph or of the overlap graph (elba_graph_components), and the gather behind the
// host's greedy partition of them (elba_partition_components, cc_partition.hpp); the rule is stated in include/elba_amd.h.
//
// Both graphs are COO on the device and are read as they lie: the overlaps as graph_input() names them (rows < cols, an edge where
// vals[].passed != 0), S in tr_out_rows / tr_out_cols.  S holds both triangles, but not always both images of a pair: the reduction
// drops an image without a direction alone.  A pair of S is an edge once, by its entry with row > column where S holds that one, else by
// the entry above the diagonal, whose image is looked up in its column (group_offsets_u32 over tr_out_cols, a binary search).  The labelling is a
// lock-free union-find in ONE pass over the edges plus pointer jumping over the reads:
//
//   k_cc_init        par[v] = v
//   k_cc_hook<G>     one lane per entry.  Both ends are walked to their roots (path splitting on the way: every read passed is pointed at
//                    its grandparent), then the LARGER root is hooked under the smaller by compare-and-swap on the larger root's own word;
//                    a lost race walks on from where it stands.  par[x] <= x always, so there is no cycle, every walk descends strictly
//                    (at most M steps; a walk that takes more sets the error word and the call fails), and the root of a finished tree is
//                    the smallest read of its component whatever the order of the edges or of the atomics: the fixed point is unique.
//                    The degrees are counted here, one add per run of equal ends among a wavefront's consecutive lanes
//   k_cc_jump        round r, one lane per read: par[v] = par[par[v]] up to CC_JUMPS times, until par[v] is a root.  In place and
//                    unordered, a launch still halves every read's depth at least (each hop of the new forest climbs two levels of the
//                    old), so the rounds are bounded by log2 of the deepest tree the hook pass left — not by the graph's diameter: a path
//                    of 2^17 + 1 reads is flat after one or two.  A round whose predecessor left nothing pending returns at once; the
//                    host queues CC_BATCH rounds per synchronisation (the protocol of sg_rounds.hpp) and gives up with
//                    ELBA_ERR_INTERNAL after CC_MAX_ROUNDS
//   k_cc_flag        flag[v] = (par[v] == v)
//   scan             exclusive_scan_u32 over flag[0 .. M]: rank[root] = the component's number (roots ascend with the smallest read),
//                    rank[M] = n
//   k_cc_reads       comp[v] = rank[par[v]], first_read, and the per-component sums over the reads (reads, bases, branches, ends)
//   k_cc_edges       the per-component sums over the edges
//   k_cc_gather      part_of_read[v] = part_of_comp[comp[v]] (elba_partition_components)
//
// Across workgroups inside a launch (k_cc_hook, k_cc_jump) every access to par[] is an agent-scope atomic: compare-and-swap / atomicMin
// for the writes, __hip_atomic_load for the walks, because the per-XCD L2s are not coherent within a launch.  Everything else crosses a
// launch boundary.  The sums are integer atomicAdds, exact in any order, behind a reduction inside the wavefront: the lanes of a wavefront
// are grouped by component (ballots), each group adds once — in an assembly that worked nearly every read names the same component, and 64
// adds to one address per wavefront would queue behind each other.  Counts come from popcounts of ballots; only the bases need shuffles.
//
// Bounds: v < M tested before every access to par / deg / flag / comp / len; an entry whose row or column is not below M is no edge; roots
// and their ranks are below M and n <= M, and the tables hold M slots each; z < nnz tested before rows / cols / vals; st[] slots CC_LIVE +
// r + 1 <= CC_ST with r < CC_MAX_ROUNDS; the look-up of an image reads ptr[r], ptr[r + 1] with r < M (M + 1 pointers, each at most nnz)
// and rows[] between them only.  No grid is capped: every kernel has one lane per read or per entry.
// Bytes moved (algorithmic): a pass over the edge list reads 16 bytes per entry (+ the `passed` byte of its 36-byte record for the
// overlaps; for S 4 bytes per step of the look-up of an entry above the diagonal) — k_cc_hook, k_cc_edges, and for S group_offsets_u32
// (8 bytes per entry); a pass over the reads moves 4 bytes per read read
// and 4 written — k_cc_init, each live k_cc_jump, k_cc_flag, the scan (8), k_cc_reads (12 + 4 for the lengths).  The hook's walks add
// 4 bytes per step; the tables are 48 bytes per read cleared, 56 bytes per component copied out.
#include "common.hpp"
#include "cc_partition.hpp"

namespace elba {

namespace {

constexpr int CC_THREADS = 256;
constexpr int CC_JUMPS = 64;                    // jumps of one lane in one k_cc_jump
constexpr int CC_BATCH = 4;                     // rounds queued between two looks at the counters
constexpr int CC_MAX_ROUNDS = 64;               // the hard cap (2^32 halved 32 times is flat)
// st[]: 0 a walk overran its bound, 1 edges, CC_LIVE + r: reads the round before r left pending (r = 0: 1)
enum { CC_ERR = 0, CC_NEDGES = 1, CC_LIVE = 8, CC_ST = CC_LIVE + CC_MAX_ROUNDS + 8 };
enum { CT_FIRST = 0, CT_READS, CT_BASES, CT_EDGES, CT_BRANCHES, CT_ENDS, CT_N };      // the tables, M slots each

using u64 = unsigned long long;

__device__ __forceinline__ uint32_t cc_load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

struct CcGraph { const int64_t *rows, *cols; const elba_overlap_t *vals; const uint32_t *ptr; int64_t nnz; uint32_t M; };

// Entry z as an edge (u > v, both below M), or none.  Every pair of S counts once: by its entry below the diagonal (row > column) where S
// holds it, else by the entry above it — the reduction can keep one image of a pair only (tr.hip: an image without a direction is
// dropped alone).  Column r of S is the entries ptr[r] .. ptr[r + 1], rows ascending: the image of (r, c) is row c of column r
template <int G>
__device__ __forceinline__ bool cc_edge(const CcGraph &g, int64_t z, uint32_t *u, uint32_t *v)
{
    if (z >= g.nnz) return false;
    const int64_t r = g.rows[z], c = g.cols[z];
    if (r < 0 || c < 0 || r >= (int64_t)g.M || c >= (int64_t)g.M || r == c) return false;
    if (G == ELBA_CC_STRING) {
        if (r < c) {
            uint32_t lo = g.ptr[r], hi = g.ptr[r + 1];      // (both at most nnz: group_offsets_u32 over nnz keys)
            while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (g.rows[mid] < c) lo = mid + 1; else hi = mid; }
            if (lo < g.ptr[r + 1] && g.rows[lo] == c) return false;
        }
    }
    else if (!g.vals[z].passed) return false;
    *u = (uint32_t)(r > c ? r : c); *v = (uint32_t)(r > c ? c : r);
    return true;
}

// The root of x, every read on the way pointed at its grandparent.  par[] descends strictly, so M steps reach a root; more: *bad.
__device__ __forceinline__ uint32_t cc_find(uint32_t *par, uint32_t x, uint32_t M, bool *bad)
{
    uint32_t p = cc_load(par + x);
    for (uint32_t step = 0; p != x; ++step) {
        if (step > M) { *bad = true; break; }
        const uint32_t g = cc_load(par + p);
        if (g != p) atomicMin(par + x, g);
        x = p; p = g;
    }
    return x;
}

// cnt[key] += the lanes of the wavefront that hold key, one add per run of equal keys among consecutive lanes; every lane must call it
__device__ __forceinline__ void cc_run_add(uint32_t *cnt, uint32_t key, bool on)
{
    const unsigned lane = threadIdx.x & 63;
    const uint32_t k = on ? key : 0xFFFFFFFFu;      // (no read has that id)
    const uint32_t prev = __shfl_up(k, 1);
    const bool head = lane == 0 || prev != k;
    const u64 hb = __ballot(head);
    if (head && on) {
        const u64 above = lane == 63 ? 0ull : hb >> (lane + 1);
        atomicAdd(cnt + key, above ? (uint32_t)__builtin_ctzll(above) + 1u : 64u - lane);
    }
}

// The lanes of a wavefront that are `on`, grouped by key: f(key, lanes of the group, its first lane) once per group, called by every lane
template <class F>
__device__ __forceinline__ void cc_groups(bool on, uint32_t key, F f)
{
    u64 rem = __ballot(on);
    while (rem) {                                  // uniform
        const int src = __builtin_ctzll(rem);
        const uint32_t k = __shfl(key, src);
        const u64 m = __ballot(on && key == k);
        f(k, m, src);
        rem &= ~m;
    }
}

__global__ void k_cc_init(uint32_t *par, uint32_t M, u64 *st)
{
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v == 0) st[CC_LIVE] = 1;
    if (v < (int64_t)M) par[v] = (uint32_t)v;
}

template <int G>
__global__ __launch_bounds__(CC_THREADS) void k_cc_hook(CcGraph g, uint32_t *par, uint32_t *deg, u64 *st)
{
    const int64_t z = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    uint32_t u = 0, v = 0;
    const bool on = cc_edge<G>(g, z, &u, &v);
    cc_run_add(deg, u, on); cc_run_add(deg, v, on);
    if (!on) return;
    uint32_t a = u, b = v;
    bool bad = false;
    for (uint32_t tries = 0;; ++tries) {
        a = cc_find(par, a, g.M, &bad);
        b = cc_find(par, b, g.M, &bad);
        if (bad || tries > g.M) { st[CC_ERR] = 1; break; }      // (every lost race is another lane's hook: there are fewer than M of those)
        if (a == b) break;
        const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
        if (atomicCAS(par + hi, hi, lo) == hi) break;
        a = hi; b = lo;
    }
}

__global__ __launch_bounds__(CC_THREADS) void k_cc_jump(uint32_t *par, uint32_t M, u64 *st, int r)
{
    if (st[CC_LIVE + r] == 0) return;
    const int64_t v = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    int pending = 0;
    if (v < (int64_t)M) {
        pending = 1;
        for (int i = 0; i < CC_JUMPS; ++i) {
            const uint32_t p = cc_load(par + v);
            const uint32_t gp = cc_load(par + p);
            if (gp == p) { pending = 0; break; }      // par[v] is a root (v itself, when p == v)
            atomicMin(par + v, gp);
        }
    }
    const u64 b = __ballot(pending);
    if (b && (threadIdx.x & 63) == (unsigned)__builtin_ctzll(b)) atomicAdd(st + CC_LIVE + r + 1, (u64)__builtin_popcountll(b));
}

__global__ void k_cc_flag(const uint32_t *par, uint32_t M, uint32_t *flag)
{
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v > (int64_t)M) return;
    flag[v] = (v < (int64_t)M && par[v] == (uint32_t)v) ? 1u : 0u;
}

__global__ __launch_bounds__(CC_THREADS) void k_cc_reads(const uint32_t *par, const uint32_t *rank, const uint32_t *deg, const uint32_t *len, uint32_t M, uint32_t base,
                                                         int32_t *comp, u64 *tab)
{
    const int64_t v = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    const unsigned lane = threadIdx.x & 63;
    const bool on = v < (int64_t)M;
    uint32_t c = 0, d = 0;
    u64 l = 0;
    if (on) {
        const uint32_t root = par[v];
        c = rank[root]; d = deg[v];
        comp[v] = (int32_t)c;
        if (root == (uint32_t)v) tab[(size_t)CT_FIRST * M + c] = (u64)v + base;
        if (len) l = len[v];
    }
    cc_groups(on, c, [&](uint32_t k, u64 m, int src) {
        const bool in = (m >> lane) & 1ull;
        const u64 nbr = __ballot(in && d > 2), nend = __ballot(in && d == 1);
        u64 sum = in ? l : 0;
        if (len) for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
        if ((int)lane == src) {
            atomicAdd(tab + (size_t)CT_READS * M + k, (u64)__builtin_popcountll(m));
            if (nbr) atomicAdd(tab + (size_t)CT_BRANCHES * M + k, (u64)__builtin_popcountll(nbr));
            if (nend) atomicAdd(tab + (size_t)CT_ENDS * M + k, (u64)__builtin_popcountll(nend));
            if (sum) atomicAdd(tab + (size_t)CT_BASES * M + k, sum);
        }
    });
}

template <int G>
__global__ __launch_bounds__(CC_THREADS) void k_cc_edges(CcGraph g, const int32_t *comp, u64 *tab, u64 *st)
{
    const int64_t z = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    const unsigned lane = threadIdx.x & 63;
    uint32_t u = 0, v = 0;
    const bool on = cc_edge<G>(g, z, &u, &v);
    const uint32_t c = on ? (uint32_t)comp[u] : 0u;
    const u64 all = __ballot(on);
    if (all && lane == (unsigned)__builtin_ctzll(all)) atomicAdd(st + CC_NEDGES, (u64)__builtin_popcountll(all));
    cc_groups(on, c, [&](uint32_t k, u64 m, int src) {
        if ((int)lane == src) atomicAdd(tab + (size_t)CT_EDGES * g.M + k, (u64)__builtin_popcountll(m));
    });
}

__global__ void k_cc_gather(const int32_t *comp, const int32_t *part_of_comp, int64_t M, int64_t n, int32_t *part_of_read)
{
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= M) return;
    const int32_t c = comp[v];
    part_of_read[v] = (c >= 0 && c < n) ? part_of_comp[c] : -1;
}

inline unsigned cc_blocks(int64_t lanes) { return (unsigned)((lanes + CC_THREADS - 1) / CC_THREADS); }

// what a labelling leaves on the host; comp[] stays on the device in c.cc.comp
struct CcTables { int64_t M = 0, n = 0; std::vector<int64_t> t[CT_N]; };

template <int G>
void cc_launch_edges(hipStream_t s, const CcGraph &g, uint32_t *par, uint32_t *deg, const int32_t *comp, u64 *tab, u64 *st, bool hook)
{
    if (hook) hipLaunchKernelGGL(k_cc_hook<G>, dim3(cc_blocks(g.nnz)), dim3(CC_THREADS), 0, s, g, par, deg, st);
    else hipLaunchKernelGGL(k_cc_edges<G>, dim3(cc_blocks(g.nnz)), dim3(CC_THREADS), 0, s, g, comp, tab, st);
}

// The labelling of cfg's graph: comp on the device, the tables on the host, the stats in c.cc.stats.
CcTables cc_label(Ctx &c, int graph, int flags, const char *who)
{
    const std::string w(who);
    ELBA_REQUIRE(graph == ELBA_CC_STRING || graph == ELBA_CC_OVERLAPS, ELBA_ERR_INVALID_ARG, w + ": unknown graph");
    ELBA_REQUIRE((flags & ~ELBA_CC_BASES) == 0, ELBA_ERR_INVALID_ARG, w + ": unknown flag");
    CcGraph g{};
    int64_t M = 0, base = 0;
    if (graph == ELBA_CC_STRING) {
        ELBA_REQUIRE(has(c.v, P_S), ELBA_ERR_STATE, w + ": no string graph (call elba_transitive_reduction)");
        M = c.tr_M; base = c.tr_id_base;
        g = CcGraph{c.tr_out_rows.as<int64_t>(), c.tr_out_cols.as<int64_t>(), nullptr, nullptr, c.tr_nnz, 0};
    } else {
        const GraphInput in = graph_input(c, who);
        M = in.M; base = in.id_base;
        g = CcGraph{in.rows, in.cols, in.vals, nullptr, in.n, 0};
    }
    const uint32_t *len = nullptr;
    if (flags & ELBA_CC_BASES) len = read_source(c, M, who, "lengths of the graph's # reads", base == 0).len;
    ELBA_REQUIRE(M < 0x7fffffffll && M + base < 0xFFFFFFFFll, ELBA_ERR_UNSUPPORTED, w + ": read ids beyond 32 bit");
    g.M = (uint32_t)M;
    c.cc.graph = -1;
    CcTables out;
    out.M = M;
    elba_cc_stats st{};
    st.nreads = M;
    if (M == 0) { c.cc.stats = st; c.cc.graph = graph; return out; }

    hipStream_t s = c.stream;
    Ctx::ComponentStage &k = c.cc;
    k.par.reserve((size_t)(M + 1) * 4); k.deg.reserve((size_t)(M + 1) * 4); k.ptr.reserve((size_t)(M + 2) * 4); k.flag.reserve((size_t)(M + 2) * 4);
    k.rank.reserve((size_t)(M + 2) * 4); k.comp.reserve((size_t)(M + 1) * 4); k.st.reserve(CC_ST * 8); k.tab.reserve((size_t)M * CT_N * 8);
    c.ws_scan.reserve((size_t)((M + 1) / 1024 + 64) * 8);
    uint32_t *par = k.par.as<uint32_t>(), *deg = k.deg.as<uint32_t>(), *ptr = k.ptr.as<uint32_t>(), *flag = k.flag.as<uint32_t>(), *rank = k.rank.as<uint32_t>();
    int32_t *comp = k.comp.as<int32_t>();
    u64 *dst = k.st.as<u64>(), *tab = k.tab.as<u64>();
    const unsigned nbM = cc_blocks(M), nbM1 = cc_blocks(M + 1);
    int passes = 0;

    k.t_total.start(s);
    k.t_label.start(s);
    ELBA_HIP(hipMemsetAsync(dst, 0, CC_ST * 8, s));
    hipLaunchKernelGGL(k_cc_init, dim3(nbM), dim3(CC_THREADS), 0, s, par, g.M, dst);
    ++passes;
    ELBA_HIP(hipMemsetAsync(deg, 0, (size_t)(M + 1) * 4, s));
    if (g.nnz > 0) {
        if (graph == ELBA_CC_STRING) {      // column pointers of S (columns ascending), for the look-up of an entry's image
            group_offsets_u32(s, reinterpret_cast<const uint64_t *>(g.cols), 0, g.nnz, ptr, M);
            g.ptr = ptr;
            ++passes;
        }
        if (graph == ELBA_CC_STRING) cc_launch_edges<ELBA_CC_STRING>(s, g, par, deg, comp, tab, dst, true);
        else cc_launch_edges<ELBA_CC_OVERLAPS>(s, g, par, deg, comp, tab, dst, true);
        ++passes;
    }
    u64 h[CC_ST] = {0};
    int queued = 0, live = 0;
    for (;;) {
        for (int r = queued; r < queued + CC_BATCH; ++r) hipLaunchKernelGGL(k_cc_jump, dim3(nbM), dim3(CC_THREADS), 0, s, par, g.M, dst, r);
        queued += CC_BATCH;
        ELBA_HIP(hipGetLastError());
        k.t_label.stop(s);
        ELBA_HIP(hipMemcpyAsync(h, dst, CC_ST * 8, hipMemcpyDeviceToHost, s));
        ELBA_HIP(hipStreamSynchronize(s));
        ELBA_REQUIRE(h[CC_ERR] == 0, ELBA_ERR_INTERNAL, w + ": a walk through the labels overran its bound");
        while (live < queued && h[CC_LIVE + live] != 0) ++live;      // the rounds that ran: a prefix
        if (live < queued || h[CC_LIVE + queued] == 0) break;
        ELBA_REQUIRE(queued + CC_BATCH <= CC_MAX_ROUNDS, ELBA_ERR_INTERNAL, w + ": the labels are not flat after " + std::to_string(queued) + " rounds");
    }
    passes += live;

    hipLaunchKernelGGL(k_cc_flag, dim3(nbM1), dim3(CC_THREADS), 0, s, par, g.M, flag);
    exclusive_scan_u32(s, flag, rank, M + 1, c.ws_scan);
    ELBA_HIP(hipMemsetAsync(tab, 0, (size_t)M * CT_N * 8, s));
    hipLaunchKernelGGL(k_cc_reads, dim3(nbM), dim3(CC_THREADS), 0, s, par, rank, deg, len, g.M, (uint32_t)base, comp, tab);
    passes += 3;
    if (g.nnz > 0) {
        if (graph == ELBA_CC_STRING) cc_launch_edges<ELBA_CC_STRING>(s, g, par, deg, comp, tab, dst, false);
        else cc_launch_edges<ELBA_CC_OVERLAPS>(s, g, par, deg, comp, tab, dst, false);
        ++passes;
    }
    ELBA_HIP(hipGetLastError());
    uint32_t n32 = 0;
    ELBA_HIP(hipMemcpyAsync(&n32, rank + M, 4, hipMemcpyDeviceToHost, s));
    ELBA_HIP(hipMemcpyAsync(h, dst, 16, hipMemcpyDeviceToHost, s));
    ELBA_HIP(hipStreamSynchronize(s));
    const int64_t n = (int64_t)n32;
    ELBA_REQUIRE(n >= 1 && n <= M, ELBA_ERR_INTERNAL, w + ": the scanned roots are not a component count");
    out.n = n;
    for (int t = 0; t < CT_N; ++t) {
        out.t[t].resize((size_t)n);
        ELBA_HIP(hipMemcpyAsync(out.t[t].data(), tab + (size_t)t * M, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    }
    k.t_total.stop(s);
    ELBA_HIP(hipStreamSynchronize(s));

    st.edges = (int64_t)h[CC_NEDGES]; st.components = n; st.passes = passes;
    int64_t best = -1, total = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t r = out.t[CT_READS][(size_t)i];
        total += r;
        if (r >= 2) ++st.used_components; else ++st.isolated;
        if (r > st.largest_reads) { st.largest_reads = r; best = i; }
    }
    ELBA_REQUIRE(total == M, ELBA_ERR_INTERNAL, w + ": the components do not hold every read once");
    if (best >= 0) st.largest_bases = out.t[CT_BASES][(size_t)best];
    st.ms_total = k.t_total.ms(); st.ms_label = k.t_label.ms();
    k.stats = st; k.graph = graph;
    return out;
}

}  // namespace

void stage_graph_components(Ctx &c, const elba_cc_cfg *cfg, elba_components_t *out)
{
    ELBA_REQUIRE(cfg, ELBA_ERR_INVALID_ARG, "graph_components: null cfg");
    ELBA_REQUIRE(cfg->reserved[0] == 0 && cfg->reserved[1] == 0, ELBA_ERR_INVALID_ARG, "graph_components: non-zero reserved word");
    const CcTables t = cc_label(c, cfg->graph, cfg->flags, "graph_components");
    out->nreads = t.M; out->n = t.n;
    out->comp_of_read = host_block<int32_t>((size_t)t.M);
    int64_t **dst[CT_N] = {&out->first_read, &out->reads, &out->bases, &out->edges, &out->branches, &out->ends};
    for (int i = 0; i < CT_N; ++i) {
        *dst[i] = host_block<int64_t>((size_t)t.n);
        if (t.n) memcpy(*dst[i], t.t[i].data(), (size_t)t.n * 8);
    }
    copy_out(c, out->comp_of_read, c.cc.comp.p, (size_t)t.M);
    ELBA_HIP(hipStreamSynchronize(c.stream));
}

void stage_partition_components(Ctx &c, const elba_part_cfg *cfg, int32_t *part_of_read, int64_t nreads, int64_t *part_weight)
{
    ELBA_REQUIRE(cfg, ELBA_ERR_INVALID_ARG, "partition_components: null cfg");
    for (int i = 0; i < 4; ++i) ELBA_REQUIRE(cfg->reserved[i] == 0, ELBA_ERR_INVALID_ARG, "partition_components: non-zero reserved word");
    ELBA_REQUIRE(cfg->nparts >= 1, ELBA_ERR_INVALID_ARG, "partition_components: nparts < 1");
    ELBA_REQUIRE(cfg->weight == 0 || cfg->weight == 1, ELBA_ERR_INVALID_ARG, "partition_components: weight is 0 (reads) or 1 (bases)");
    ELBA_REQUIRE(cfg->min_reads >= 0, ELBA_ERR_INVALID_ARG, "partition_components: negative min_reads");
    ELBA_REQUIRE(part_weight && (part_of_read || nreads == 0), ELBA_ERR_INVALID_ARG, "partition_components: null output");
    const CcTables t = cc_label(c, cfg->graph, cfg->weight ? ELBA_CC_BASES : 0, "partition_components");
    ELBA_REQUIRE(nreads == t.M, ELBA_ERR_INVALID_ARG, "partition_components: need one entry per read of the graph");
    std::vector<int32_t> poc;
    std::vector<int64_t> pw;
    cc_partition(t.t[CT_READS].data(), t.t[cfg->weight ? CT_BASES : CT_READS].data(), t.n, cfg->nparts, cfg->min_reads, poc, pw);
    memcpy(part_weight, pw.data(), (size_t)cfg->nparts * 8);
    if (t.M == 0) return;
    hipStream_t s = c.stream;
    c.cc.pcomp.reserve((size_t)t.n * 4); c.cc.pread.reserve((size_t)t.M * 4);
    ELBA_HIP(hipMemcpyAsync(c.cc.pcomp.p, poc.data(), (size_t)t.n * 4, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_cc_gather, dim3(cc_blocks(t.M)), dim3(CC_THREADS), 0, s, c.cc.comp.as<int32_t>(), c.cc.pcomp.as<int32_t>(), t.M, t.n, c.cc.pread.as<int32_t>());
    ELBA_HIP(hipGetLastError());
    copy_out(c, part_of_read, c.cc.pread.p, (size_t)t.M);
    ELBA_HIP(hipStreamSynchronize(s));
}

}  // namespace elba
