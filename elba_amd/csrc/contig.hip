// contig.hip — from the string graph to contig sequences: what GenerateContigs (src/ContigGeneration.cpp:18-51,110,376-457) does on one
// rank, and the strings parallel_write_contigs (src/main.cpp:487-512) writes.
//
// Input: the S that tr.hip leaves on the context (tr_out_*), both triangles, column-major — entry (row r, col c) carries S(r, c), the
// Overlap whose Q read is r.  Column c therefore lists c's neighbours ascending, and the entry the reference's walk reads at c,
// S(c, r) = Overlap::Transpose of the stored S(r, c): its suffixT is the stored suffix, its direction the stored directionT.  No transpose
// pass, no sort: degrees are column lengths (D.Reduce(Row) on the symmetric S, :31-32).
//
//   k_cg_adjacency    deg > 2 marks a branch (:39); every other read keeps its at most two non-branch neighbours (PruneFull, :44), column
//                     order, with the walk's suffixT / direction of S(v, r) and the direction of S(r, v) (what the walk carries in
//                     `lastdir` when it arrives at v)
//   k_cg_arcs         each kept edge is two arcs; succ(u->v) = v->w, w v's other neighbour (none: v has one neighbour, the arc is terminal)
//   k_cg_jump x R     Wyllie pointer jumping, R = ceil(log2 M) rounds, double-buffered: far = the arc reached, rank = arcs to it, mn = the
//                     smallest head on the way.  An arc whose far arc still has a successor lies on a cycle.
//   k_cg_vertices     per read of a path: its start (the smaller degree-1 end — the walk's v, :406-409), its place in the chain (rank of
//                     the arc back to the start + 1), the chain length at the start; a cycle's smallest read counts it
//   scans             contig ids over the starts, chain offsets over the chain lengths (ascending start = the walk's emission order)
//   k_cg_elements     chain elements (:437-452): read, prefix = suffixT of the outgoing S(cur, next) or len for the last, strand bit;
//                     a prefix outside [0, len] is recorded (the smallest (read, next) pair) and fails the call
//   scan              base offsets of the elements (i64)
//   k_cg_contigs      per contig: sequence and chain offsets, the longest contig; totals for the host
//   -- the one host synchronisation: the output size --
//   k_cg_write        one wavefront per element: 2-bit packed bases -> ASCII, reverse complement on the strand bit; lanes own 8-byte
//                     aligned words of the output, whole words go out as one 8-byte store, the two boundary words bytewise
//
// Two opt-in extensions (elba_generate_contigs_ex; with flags 0 nothing below is launched and the sequence above is unchanged):
//
//   ELBA_CONTIG_CIRCULAR    pointer jumping cannot rank a cycle, so it is cut: after the R rounds k_cg_cut rebuilds the initial arcs with
//                           every arc whose head is its cycle's smallest read s (mn of the first pass, which stays untouched) terminal,
//                           and k_cg_jump2 x R ranks the cut cycles (far, rank; arcs off every cycle and the cut arcs are fixed points
//                           written to both buffers once and skipped; every round returns at once when k_cg_cut counted no cut arc on
//                           the device, the host does not wait for that count).  Both arcs leaving a cycle read now reach a terminal arc into s; the one
//                           that points along the walk (s -> its smaller neighbour -> ...) ends in the arc whose tail is s's larger
//                           neighbour.  Cycle length = rank of s's chosen arc + 1, place in the chain = length - 1 - rank, outgoing slot =
//                           the chosen arc's, for the last read too (its next is s): every element follows the interior rule, the
//                           contig closes on itself.  No strand-consistency check (the reference makes none on paths either).
//   ELBA_CONTIG_SINGLETONS  a read with no kept neighbour (isolated, or a branch) whose read flags are 0 and whose length is not 0 is a
//                           chain of its own: (v, len, strand 0).
//
// The starts of all three kinds set `flag`, so the scans merge them by ascending start read; k_cg_contigs writes each contig's kind.
// The second ranking pass moves 2 x 4 bytes x 2 x 2M per round when cycles exist (it carries no mn), against the first pass's
// 3 x 4 bytes x 2 x 2M; 4 bytes x 2M per round for a graph whose arcs are all off cycles would be read if the count did not end the round first.
//
// Bounds: every index into S is below tr_nnz, every vertex index below M, arc ids below 2M, chain elements below M (a read is in at most
// one chain), base offsets below the total the scan returns, which sizes the output.  Bytes moved (algorithmic): S once (8 + 36 bytes per
// entry, the rows / values of the at most two entries of a non-branch column), 3 x 4 bytes x 2 x 2M per jump round, O(M) for the scans,
// and per base a quarter byte read + one byte written.
#include "common.hpp"

namespace elba {

namespace {

struct alignas(16) CgSlot {
    uint32_t nb;        // the neighbour r
    int32_t sfx;        // suffixT of S(v, r) = the stored S(r, v).suffix
    int32_t dwalk;      // direction of S(v, r) = the stored directionT
    int32_t din;        // direction of S(r, v) = the stored direction
};

constexpr uint32_t CG_NONE = 0xffffffffu;

// counters: 0 branches, 1 isolated non-branch reads, 2 cycles, 3 smallest bad (read << 32 | next), 4 contigs, 5 elements, 6 bases, 7 longest
__global__ void k_cg_adjacency(const uint32_t *ptr, const int64_t *rows, const elba_overlap_t *vals, uint32_t M, CgSlot *slot, uint8_t *kdeg,
                               unsigned long long *ctr)
{
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    bool branch = false, single = false;
    if (v < M) {
        const uint32_t s = ptr[v], d = ptr[v + 1] - s;
        branch = d > 2;
        uint32_t k = 0;
        if (!branch)
            for (uint32_t t = 0; t < d; ++t) {
                const uint32_t r = (uint32_t)rows[s + t];
                if (r >= M || ptr[r + 1] - ptr[r] > 2) continue;
                const elba_overlap_t o = vals[s + t];
                slot[2 * v + k] = CgSlot{r, o.suffix, (int32_t)o.directionT, (int32_t)o.direction};
                ++k;
            }
        kdeg[v] = (uint8_t)k;
        single = !branch && k == 0;
    }
    const unsigned long long bb = __ballot(branch), bs = __ballot(single);
    const unsigned lane = threadIdx.x & 63;
    if (bb && lane == (unsigned)__builtin_ctzll(bb)) atomicAdd(&ctr[0], (unsigned long long)__builtin_popcountll(bb));
    if (bs && lane == (unsigned)__builtin_ctzll(bs)) atomicAdd(&ctr[1], (unsigned long long)__builtin_popcountll(bs));
}

// arc a = 2 v + k: v -> slot[a].nb; arcs with k >= kdeg[v] do not exist (far = itself, never read by a real arc)
__global__ void k_cg_arcs(const CgSlot *slot, const uint8_t *kdeg, uint32_t M, uint32_t *far, uint32_t *rank, uint32_t *mn, uint8_t *term)
{
    const uint32_t a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= 2 * M) return;
    const uint32_t v = a >> 1, k = a & 1u;
    if (k >= kdeg[v]) { far[a] = a; rank[a] = 0; mn[a] = CG_NONE; term[a] = 1; return; }
    const uint32_t w = slot[a].nb;
    uint32_t succ = CG_NONE;
    if (kdeg[w] == 2) {                                     // leave w by its other neighbour (S is symmetric: one of w's slots names v)
        if (slot[2 * w].nb == v) succ = 2 * w + 1;
        else if (slot[2 * w + 1].nb == v) succ = 2 * w;
    }
    far[a] = succ == CG_NONE ? a : succ;
    rank[a] = succ == CG_NONE ? 0u : 1u;
    mn[a] = w;
    term[a] = succ == CG_NONE ? 1 : 0;
}

__global__ void k_cg_jump(uint32_t n, const uint32_t *far0, const uint32_t *rank0, const uint32_t *mn0, uint32_t *far1, uint32_t *rank1, uint32_t *mn1)
{
    const uint32_t a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= n) return;
    const uint32_t f = far0[a];
    const uint32_t m0 = mn0[a], m1 = mn0[f];
    far1[a] = far0[f];
    rank1[a] = rank0[a] + rank0[f];
    mn1[a] = m0 < m1 ? m0 : m1;
}

// CIRCULAR: the initial arcs again, cut at every cycle's smallest read.  far / mn: the first pass's result (read only).  A cycle arc whose
// head is mn becomes terminal; arcs that need no ranking (off every cycle, cut, absent) are fixed points in both buffers.  ctr[8]: cut arcs.
__global__ void k_cg_cut(const CgSlot *slot, const uint8_t *kdeg, const uint32_t *far, const uint32_t *mn, const uint8_t *term, uint32_t M,
                         uint32_t *cfar0, uint32_t *crank0, uint32_t *cfar1, uint32_t *crank1, unsigned long long *ctr)
{
    const uint32_t a = blockIdx.x * blockDim.x + threadIdx.x;
    bool cut = false;
    if (a < 2 * M) {
        const uint32_t v = a >> 1, k = a & 1u;
        uint32_t succ = CG_NONE;
        if (k < kdeg[v] && !term[far[a]]) {                     // a cycle arc: both ends have two kept neighbours
            const uint32_t w = slot[a].nb;
            cut = w == mn[a];
            if (!cut) succ = slot[2 * w].nb == v ? 2 * w + 1 : 2 * w;
        }
        if (succ == CG_NONE) { cfar0[a] = a; crank0[a] = 0; cfar1[a] = a; crank1[a] = 0; }
        else { cfar0[a] = succ; crank0[a] = 1; }
    }
    const unsigned long long b = __ballot(cut);
    if (b && (threadIdx.x & 63) == (unsigned)__builtin_ctzll(b)) atomicAdd(&ctr[8], (unsigned long long)__builtin_popcountll(b));
}

__global__ void k_cg_jump2(uint32_t n, const uint32_t *far0, const uint32_t *rank0, uint32_t *far1, uint32_t *rank1, const unsigned long long *ctr)
{
    if (ctr[8] == 0) return;                                    // no cycle: every arc is a fixed point in both buffers
    const uint32_t a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= n) return;
    const uint32_t f = far0[a];
    if (f == a) return;
    far1[a] = far0[f];
    rank1[a] = rank0[a] + rank0[f];
}

// vinfo[v] = {start, place in the chain, slot of the outgoing edge (CG_NONE: last element)}; flag / nel at the starts
// vinfo.w = the kind of v's contig (0 path, 1 circular, 2 single read).  cfar / crank: the ranks of the cut cycles (CIRCULAR only);
// rflags / len: the read flags of the transitive reduction and the read lengths (SINGLETONS only)
__global__ void k_cg_vertices(const CgSlot *slot, const uint8_t *kdeg, const uint32_t *far, const uint32_t *rank, const uint32_t *mn, const uint8_t *term,
                              uint32_t M, uint4 *vinfo, uint32_t *flag, uint32_t *nel, unsigned long long *ctr, int cflags, const uint32_t *cfar,
                              const uint32_t *crank, const uint8_t *rflags, const uint32_t *len)
{
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    bool cycle_head = false;
    if (v < M) {
        const uint32_t kd = kdeg[v];
        uint4 info = make_uint4(CG_NONE, 0, CG_NONE, 0);
        uint32_t f = 0, n = 0;
        if (kd > 0) {
            const uint32_t f0 = far[2 * v];
            if (!term[f0]) {                                        // on a cycle: no degree-1 read, the walk never starts there
                const uint32_t s = mn[2 * v];
                cycle_head = kd == 2 && s == v;
                if (cflags & ELBA_CONTIG_CIRCULAR) {                // the walk leaves s towards its smaller neighbour and comes back by the larger
                    const uint32_t n0 = slot[2 * s].nb, n1 = slot[2 * s + 1].nb;
                    const uint32_t hi = n0 < n1 ? n1 : n0, sarc = 2 * s + (n0 < n1 ? 0u : 1u);
                    const uint32_t out = (cfar[2 * v] >> 1) == hi ? 0u : 1u;        // the arc whose terminal arc leaves s's larger neighbour
                    const uint32_t L = crank[sarc] + 1;
                    info = make_uint4(s, L - 1 - crank[2 * v + out], out, 1);
                    if (v == s) { f = 1; n = L; }
                }
            } else {
                const uint32_t e0 = slot[f0].nb;
                const uint32_t e1 = kd == 2 ? slot[far[2 * v + 1]].nb : v;      // the two ends of the path (v itself when it is one)
                const uint32_t s = e0 < e1 ? e0 : e1;
                uint32_t pos = 0, out = CG_NONE;
                if (v == s) { out = 0; f = 1; n = rank[2 * v] + 2; }
                else if (kd == 1) pos = rank[2 * v] + 1;                        // the other end: last element
                else if (e0 == s) { pos = rank[2 * v] + 1; out = 1; }
                else { pos = rank[2 * v + 1] + 1; out = 0; }
                info = make_uint4(s, pos, out, 0);
            }
        } else if ((cflags & ELBA_CONTIG_SINGLETONS) && rflags[v] == 0 && len[v] != 0) {     // no kept neighbour (isolated or a branch), neither bad nor contained
            info = make_uint4(v, 0, CG_NONE, 2); f = 1; n = 1;
        }
        vinfo[v] = info; flag[v] = f; nel[v] = n;
    } else if (v == M) { flag[v] = 0; nel[v] = 0; }
    const unsigned long long b = __ballot(cycle_head);
    if (b && (threadIdx.x & 63) == (unsigned)__builtin_ctzll(b)) atomicAdd(&ctr[2], (unsigned long long)__builtin_popcountll(b));
}

__global__ void k_cg_elements(const CgSlot *slot, const uint4 *vinfo, const uint32_t *cidx, const uint32_t *eoff, const uint32_t *len, uint32_t M, int64_t base,
                              int32_t *cid, int64_t *eread, int32_t *epre, uint8_t *estr, unsigned long long *ctr)
{
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= M) return;
    const uint4 info = vinfo[v];
    if (info.x == CG_NONE) { cid[v] = -1; return; }
    const uint32_t s = info.x, el = eoff[s] + info.y;
    cid[v] = (int32_t)cidx[s];
    eread[el] = (int64_t)v + base;
    const int32_t L = (int32_t)len[v];
    int32_t prefix; int strand;
    if (info.z != CG_NONE) {
        const CgSlot o = slot[2 * v + info.z];
        prefix = o.sfx; strand = (o.dwalk >> 1) & 1;                   // (o.direction >> 1) & 1, :437
        if (prefix < 0 || prefix > L) { atomicMin(&ctr[3], ((unsigned long long)v << 32) | o.nb); prefix = 0; }
    } else {
        prefix = L; strand = info.w == 2 ? 0 : 1 - (slot[2 * v].din & 1);      // 1 - (lastdir & 1), :450; a single read as it is
    }
    epre[el] = prefix; estr[el] = (uint8_t)strand;
}

// ctr[9] circular contigs, ctr[10] single-read contigs
__global__ void k_cg_contigs(const uint32_t *flag, const uint32_t *cidx, const uint32_t *eoff, const uint32_t *nel, const int64_t *eboff, const uint4 *vinfo, uint32_t M,
                             int64_t *soff, int64_t *coff, uint8_t *kind, unsigned long long *ctr)
{
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t kd = 0;
    if (v == M) {
        const uint32_t nc = cidx[M], E = eoff[M];
        soff[nc] = eboff[E]; coff[nc] = E;
        ctr[4] = nc; ctr[5] = E; ctr[6] = (unsigned long long)eboff[E];
    } else if (v < M && flag[v]) {
        const uint32_t k = cidx[v], e = eoff[v];
        const int64_t b0 = eboff[e], b1 = eboff[e + nel[v]];
        soff[k] = b0; coff[k] = e;
        kd = vinfo[v].w;
        kind[k] = (uint8_t)kd;
        atomicMax(&ctr[7], (unsigned long long)(b1 - b0));
    }
    const unsigned long long bc = __ballot(kd == 1), bs = __ballot(kd == 2);
    const unsigned lane = threadIdx.x & 63;
    if (bc && lane == (unsigned)__builtin_ctzll(bc)) atomicAdd(&ctr[9], (unsigned long long)__builtin_popcountll(bc));
    if (bs && lane == (unsigned)__builtin_ctzll(bs)) atomicAdd(&ctr[10], (unsigned long long)__builtin_popcountll(bs));
}

__device__ __forceinline__ uint32_t cg_base(const uint8_t *mem, uint32_t i) { return (mem[i >> 2] >> (6 - 2 * (i & 3))) & 3u; }   // src/DnaSeq.cpp:48-54

constexpr int CG_WRITE_THREADS = 256;
__global__ __launch_bounds__(CG_WRITE_THREADS) void k_cg_write(const int64_t *eread, const int32_t *epre, const uint8_t *estr, const int64_t *eboff, int64_t E,
                                                               int64_t base, const uint8_t *packed, const uint64_t *byte_off, const uint32_t *len, char *out)
{
    const unsigned lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * (CG_WRITE_THREADS / 64);
    for (int64_t e = (int64_t)blockIdx.x * (CG_WRITE_THREADS / 64) + (threadIdx.x >> 6); e < E; e += waves) {
        const int64_t p = epre[e];
        if (p <= 0) continue;
        const uint32_t r = (uint32_t)(eread[e] - base);
        const bool rc = estr[e] != 0;
        const uint8_t *src = packed + byte_off[r];
        const uint32_t L = len[r];
        const int64_t lo = eboff[e], hi = lo + p;
        const int64_t w0 = lo >> 3, w1 = (hi - 1) >> 3;
        for (int64_t w = w0 + lane; w <= w1; w += 64) {
            const int64_t o0 = w << 3;
            if (o0 >= lo && o0 + 8 <= hi) {
                uint64_t word = 0;
#pragma unroll
                for (int b = 0; b < 8; ++b) {
                    const uint32_t i = (uint32_t)(o0 + b - lo);
                    const uint32_t code = rc ? 3u - cg_base(src, L - 1 - i) : cg_base(src, i);
                    word |= (uint64_t)(uint8_t)"ACGT"[code] << (8 * b);
                }
                *reinterpret_cast<uint64_t *>(out + o0) = word;
            } else {
                for (int b = 0; b < 8; ++b) {
                    const int64_t o = o0 + b;
                    if (o < lo || o >= hi) continue;
                    const uint32_t i = (uint32_t)(o - lo);
                    const uint32_t code = rc ? 3u - cg_base(src, L - 1 - i) : cg_base(src, i);
                    out[o] = "ACGT"[code];
                }
            }
        }
    }
}

}  // namespace

void stage_generate_contigs(Ctx &c, int flags)
{
    enter(c.v, EV_GENERATE_CONTIGS);
    ELBA_REQUIRE((flags & ~(ELBA_CONTIG_CIRCULAR | ELBA_CONTIG_SINGLETONS)) == 0, ELBA_ERR_INVALID_ARG, "generate_contigs: unknown flag bits");
    ELBA_REQUIRE(has(c.v, P_S), ELBA_ERR_STATE, "generate_contigs: no string graph (call elba_transitive_reduction)");
    const int64_t M = c.tr_M, nnz = c.tr_nnz;
    // (the replicated set is indexed by global read id, the graph by row: the same reads only when the graph's ids have no base)
    const ReadSource src = read_source(c, M, "generate_contigs", "sequences of the graph's # reads", c.tr_id_base == 0);
    const uint8_t *packed = src.packed; const uint64_t *byte_off = src.byte_off; const uint32_t *len = src.len;
    accepted(c.v, EV_GENERATE_CONTIGS);
    hipStream_t s = c.stream;
    const int64_t base = c.tr_id_base;
    elba_contig_stats st{};
    st.nreads = M;
    int R = 0;
    while ((1ll << R) < M) ++R;                                 // arc chains are shorter than M: 2^R >= M covers every path and cycle
    // every buffer of the launch sequence before the first launch (the output is sized after the one synchronisation)
    c.cg.ptr.reserve((size_t)(M + 2) * 4); c.cg.slot.reserve((size_t)(2 * M + 2) * sizeof(CgSlot)); c.cg.kdeg.reserve((size_t)M + 4);
    for (int b = 0; b < 2; ++b) { c.cg.far[b].reserve((size_t)(2 * M + 2) * 4); c.cg.rank[b].reserve((size_t)(2 * M + 2) * 4); c.cg.mn[b].reserve((size_t)(2 * M + 2) * 4); }
    c.cg.term.reserve((size_t)2 * M + 4); c.cg.vinfo.reserve((size_t)(M + 1) * sizeof(uint4));
    c.cg.flag.reserve((size_t)(M + 2) * 4); c.cg.cidx.reserve((size_t)(M + 2) * 4); c.cg.nel.reserve((size_t)(M + 2) * 4); c.cg.eoff.reserve((size_t)(M + 2) * 4);
    c.cg.cid.reserve((size_t)(M + 1) * 4); c.cg.eread.reserve((size_t)(M + 1) * 8); c.cg.epre.reserve((size_t)(M + 2) * 4); c.cg.estr.reserve((size_t)M + 4);
    c.cg.eboff.reserve((size_t)(M + 2) * 8); c.cg.soff.reserve((size_t)(M + 2) * 8); c.cg.coff.reserve((size_t)(M + 2) * 8); c.cg.ctr.reserve(128);
    c.cg.kind.reserve((size_t)M + 4);
    const bool circular = (flags & ELBA_CONTIG_CIRCULAR) != 0;
    if (circular)                                               // the second ranking pass reads the first one's far / mn / term, which stay as they are
        for (int b = 0; b < 2; ++b) { c.cg.cfar[b].reserve((size_t)(2 * M + 2) * 4); c.cg.crank[b].reserve((size_t)(2 * M + 2) * 4); }
    uint32_t *ptr = c.cg.ptr.as<uint32_t>(); CgSlot *slot = c.cg.slot.as<CgSlot>(); uint8_t *kdeg = c.cg.kdeg.as<uint8_t>(), *term = c.cg.term.as<uint8_t>();
    unsigned long long *ctr = c.cg.ctr.as<unsigned long long>();
    c.cg.t_total.start(s);
    ELBA_HIP(hipMemsetAsync(ctr, 0, 128, s));
    ELBA_HIP(hipMemsetAsync(ctr + 3, 0xff, 8, s));
    ELBA_HIP(hipMemsetAsync(c.cg.epre.p, 0, (size_t)(M + 2) * 4, s));
    const unsigned nbM = (unsigned)((M + 1 + 255) / 256), nbA = (unsigned)((2 * M + 255) / 256);
    if (nnz > 0) group_offsets_u32(s, reinterpret_cast<const uint64_t *>(c.tr_out_cols.p), 0, nnz, ptr, M);     // column pointers of S (columns ascending)
    else ELBA_HIP(hipMemsetAsync(ptr, 0, (size_t)(M + 1) * 4, s));
    int which = 0;
    if (M > 0) {
        hipLaunchKernelGGL(k_cg_adjacency, dim3(nbM), dim3(256), 0, s, ptr, c.tr_out_rows.as<int64_t>(), c.tr_out_vals.as<elba_overlap_t>(), (uint32_t)M, slot, kdeg, ctr);
        hipLaunchKernelGGL(k_cg_arcs, dim3(nbA), dim3(256), 0, s, slot, kdeg, (uint32_t)M, c.cg.far[0].as<uint32_t>(), c.cg.rank[0].as<uint32_t>(), c.cg.mn[0].as<uint32_t>(), term);
    }
    c.cg.t_rank.start(s);
    if (M > 0) {
        for (int r = 0; r < R; ++r, which ^= 1)
            hipLaunchKernelGGL(k_cg_jump, dim3(nbA), dim3(256), 0, s, (uint32_t)(2 * M), c.cg.far[which].as<uint32_t>(), c.cg.rank[which].as<uint32_t>(), c.cg.mn[which].as<uint32_t>(),
                               c.cg.far[which ^ 1].as<uint32_t>(), c.cg.rank[which ^ 1].as<uint32_t>(), c.cg.mn[which ^ 1].as<uint32_t>());
    }
    int cwhich = 0;
    if (circular && M > 0) {
        hipLaunchKernelGGL(k_cg_cut, dim3(nbA), dim3(256), 0, s, slot, kdeg, c.cg.far[which].as<uint32_t>(), c.cg.mn[which].as<uint32_t>(), term, (uint32_t)M,
                           c.cg.cfar[0].as<uint32_t>(), c.cg.crank[0].as<uint32_t>(), c.cg.cfar[1].as<uint32_t>(), c.cg.crank[1].as<uint32_t>(), ctr);
        for (int r = 0; r < R; ++r, cwhich ^= 1)
            hipLaunchKernelGGL(k_cg_jump2, dim3(nbA), dim3(256), 0, s, (uint32_t)(2 * M), c.cg.cfar[cwhich].as<uint32_t>(), c.cg.crank[cwhich].as<uint32_t>(),
                               c.cg.cfar[cwhich ^ 1].as<uint32_t>(), c.cg.crank[cwhich ^ 1].as<uint32_t>(), ctr);
    }
    c.cg.t_rank.stop(s);
    uint32_t *flag = c.cg.flag.as<uint32_t>(), *cidx = c.cg.cidx.as<uint32_t>(), *nel = c.cg.nel.as<uint32_t>(), *eoff = c.cg.eoff.as<uint32_t>();
    hipLaunchKernelGGL(k_cg_vertices, dim3(nbM), dim3(256), 0, s, slot, kdeg, c.cg.far[which].as<uint32_t>(), c.cg.rank[which].as<uint32_t>(), c.cg.mn[which].as<uint32_t>(), term,
                       (uint32_t)M, c.cg.vinfo.as<uint4>(), flag, nel, ctr, flags, circular ? c.cg.cfar[cwhich].as<uint32_t>() : nullptr,
                       circular ? c.cg.crank[cwhich].as<uint32_t>() : nullptr, c.tr_flags.as<uint8_t>(), len);
    exclusive_scan_u32(s, flag, cidx, M + 1, c.ws_scan);
    exclusive_scan_u32(s, nel, eoff, M + 1, c.ws_scan);
    if (M > 0)
        hipLaunchKernelGGL(k_cg_elements, dim3(nbM), dim3(256), 0, s, slot, c.cg.vinfo.as<uint4>(), cidx, eoff, len, (uint32_t)M, base, c.cg.cid.as<int32_t>(),
                           c.cg.eread.as<int64_t>(), c.cg.epre.as<int32_t>(), c.cg.estr.as<uint8_t>(), ctr);
    exclusive_scan_u32_to_i64(s, c.cg.epre.as<uint32_t>(), c.cg.eboff.as<int64_t>(), M + 1, c.ws_scan);     // prefixes are >= 0 here (bad ones were zeroed)
    hipLaunchKernelGGL(k_cg_contigs, dim3(nbM), dim3(256), 0, s, flag, cidx, eoff, nel, c.cg.eboff.as<int64_t>(), c.cg.vinfo.as<uint4>(), (uint32_t)M,
                       c.cg.soff.as<int64_t>(), c.cg.coff.as<int64_t>(), c.cg.kind.as<uint8_t>(), ctr);
    ELBA_HIP(hipGetLastError());
    unsigned long long h[16] = {0};
    ELBA_HIP(hipMemcpyAsync(h, ctr, 128, hipMemcpyDeviceToHost, s));
    ELBA_HIP(hipStreamSynchronize(s));
    if (h[3] != ~0ull) {
        const uint32_t v = (uint32_t)(h[3] >> 32), r = (uint32_t)h[3];
        CgSlot hs[2]; uint32_t L = 0;
        ELBA_HIP(hipMemcpyAsync(hs, slot + 2 * (size_t)v, sizeof(hs), hipMemcpyDeviceToHost, s));
        ELBA_HIP(hipMemcpyAsync(&L, len + v, 4, hipMemcpyDeviceToHost, s));
        ELBA_HIP(hipStreamSynchronize(s));
        const int32_t pre = hs[0].nb == r ? hs[0].sfx : hs[1].sfx;
        throw Error{ELBA_ERR_INVALID_ARG, "generate_contigs: the chain element of read " + std::to_string((int64_t)v + base) + " (next read " + std::to_string((int64_t)r + base) +
                                              ") takes a prefix of " + std::to_string(pre) + " bases, outside [0, " + std::to_string(L) + "]: suffixT of S(" +
                                              std::to_string((int64_t)v + base) + ", " + std::to_string((int64_t)r + base) + ") is not a valid prefix length"};
    }
    const int64_t nc = (int64_t)h[4], E = (int64_t)h[5], bases = (int64_t)h[6];
    c.cg.seq.reserve((size_t)bases + 64);
    if (E > 0 && bases > 0) {
        int64_t grid = (E + CG_WRITE_THREADS / 64 - 1) / (CG_WRITE_THREADS / 64);
        if (grid > (int64_t)c.num_cus * 16) grid = (int64_t)c.num_cus * 16;
        hipLaunchKernelGGL(k_cg_write, dim3((unsigned)grid), dim3(CG_WRITE_THREADS), 0, s, c.cg.eread.as<int64_t>(), c.cg.epre.as<int32_t>(), c.cg.estr.as<uint8_t>(),
                           c.cg.eboff.as<int64_t>(), E, base, packed, byte_off, len, c.cg.seq.as<char>());
        ELBA_HIP(hipGetLastError());
    }
    c.cg.t_total.stop(s);
    ELBA_HIP(hipStreamSynchronize(s));
    const int64_t ncirc = (int64_t)h[9], nsingle = (int64_t)h[10];
    st.branches = (int64_t)h[0]; st.cycles = (int64_t)h[2]; st.contigs = nc;
    st.used_components = nc - ncirc - nsingle + st.cycles;                  // paths + cycles, whether the cycles were emitted or not
    st.components = st.branches + (int64_t)h[1] + st.used_components;     // CC on S without the branches' rows and columns: a branch read is a component of its own
    st.contig_reads = E; st.bases = bases; st.longest = (int64_t)h[7];
    st.ms_total = c.cg.t_total.ms(); st.ms_rank = c.cg.t_rank.ms();
    c.cg.n = nc; c.cg.E = E; c.cg.bases = bases; c.cg.circular = ncirc; c.cg.singletons = nsingle; c.cg.stats = st; ++c.cg.serial; done(c.v, EV_GENERATE_CONTIGS);
}

void stage_generate_contigs_ex(Ctx &c, const elba_contig_cfg *cfg)
{
    enter(c.v, EV_GENERATE_CONTIGS);                            // (before the checks: a rejected call leaves no contigs either; entered again below, which changes nothing)
    ELBA_REQUIRE(cfg, ELBA_ERR_INVALID_ARG, "generate_contigs_ex: null cfg");
    ELBA_REQUIRE(!cfg->reserved[0] && !cfg->reserved[1] && !cfg->reserved[2], ELBA_ERR_INVALID_ARG, "generate_contigs_ex: reserved words must be 0");
    ELBA_REQUIRE((cfg->flags & ~(ELBA_CONTIG_CIRCULAR | ELBA_CONTIG_SINGLETONS)) == 0, ELBA_ERR_INVALID_ARG, "generate_contigs_ex: unknown flag bits");
    stage_generate_contigs(c, cfg->flags);
}

}  // namespace elba
