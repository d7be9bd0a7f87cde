// graph_links.hip — from the string graph and its contigs to the links of the assembly graph (elba_export_assembly_links; the rule is
// stated in include/elba_amd.h): which contig ends meet at a branch read, in which orientation, with how many bases of overlap.
//
// Input, all resident: S as tr.hip leaves it (tr_out_*: both triangles, column-major, the entry at (row v, column u) is S(v, u), so the
// step u -> v the contig walk reads at u is its transpose: prefix = the stored suffix, direction = the stored directionT, and the step
// v -> u is the stored suffixT / direction); of the last contig call the read map cg.cid (contig of every read, -1: none — kept by the
// contig stage and read as it is), the chain arrays cg.eread / cg.estr / cg.coff, the kinds and the sequence offsets; the read lengths.
//
//   k_gl_bits       one lane per chain element: first / last / strand bits of its read (the contig of a read is cg.cid, not recomputed)
//   k_gl_links<0>   the count pass.  A wavefront takes 64 consecutive columns.  A column of up to 64 entries is walked by its lane (its
//                   rows below the diagonal: v > u).  A longer column is worked on by the whole wavefront afterwards, 64 entries a trip,
//                   the kept entries placed by ballot + popcount.  cnt[u] = records of column u, the closure record of a circular contig
//                   that starts at u included (it sorts at (u, u), in front of every (u, v)); the counters of the stats, added up per
//                   workgroup and stored, no atomics
//   k_gl_sum        one workgroup adds the workgroups' counters up
//   scan            exclusive_scan_u32 over cnt[0 .. M]: off[u] = the first record of column u, off[M] the total
//   -- the one host synchronisation: the output size (and the counters) --
//   k_gl_links<1>   the emit pass: the same walk, records written at off[u] + (closure) + place.  Columns ascend and rows ascend within a
//                   column, so the records come out sorted by (from_read, to_read) without a sort
//
// Bounds: column pointers come from group_offsets_u32 over tr_nnz keys, so every index into S is below tr_nnz; a row >= M is skipped, so
// reads are below M wherever they index ptr / cid / bits / len; a contig index is read only when cid >= 0 and is below the contig count
// (soff has count + 1 entries); a record index is off[u] + place with place < cnt[u], hence below off[M], which sizes the output.
// Bytes moved (algorithmic): per pass the lower triangle of S (8 + 36 bytes per entry; a column that is neither a branch nor holds a
// branch row stops at the degrees), 4 + 4 + 1 bytes per read, and 24 bytes per record written once.
#include "common.hpp"

namespace elba {

namespace {

constexpr int GL_THREADS = 256;
constexpr uint32_t GL_LANE_MAX = 64;      // longer columns go to the whole wavefront

enum { GL_FIRST = 1, GL_LAST = 2, GL_STRAND = 4 };
// counters: 0 candidates, 1 links, 2 closures, 3 twisted, 4 unplaced, 5 clamped, 6 asymmetric
enum { GC_CAND = 0, GC_LINKS, GC_CLOS, GC_TWIST, GC_UNPL, GC_CLAMP, GC_ASYM, GC_N };

struct GlIn {
    const uint32_t *ptr; const int64_t *rows; const elba_overlap_t *vals;      // S
    const int32_t *cid; const uint8_t *bits, *kind; const int64_t *soff;       // contigs
    const uint32_t *len;
    uint32_t M, base;
};

__global__ void k_gl_bits(const int64_t *eread, const uint8_t *estr, const int64_t *coff, const int32_t *cid, int64_t E, int64_t base, uint32_t M, uint8_t *bits)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const int64_t r = eread[e] - base;
    if (r < 0 || r >= (int64_t)M) return;
    const int32_t k = cid[r];
    if (k < 0) return;
    bits[r] = (uint8_t)((e == coff[k] ? GL_FIRST : 0) | (e == coff[k + 1] - 1 ? GL_LAST : 0) | (estr[e] ? GL_STRAND : 0));
}

// one entry of column u (row v > u, v < M): -1 no candidate, else its counter; a link's record in *rec
__device__ __forceinline__ int gl_classify(const GlIn &g, uint32_t u, uint32_t du, uint32_t v, const elba_overlap_t &o, elba_link_t *rec, bool *clamped, bool *asym)
{
    const uint32_t dv = g.ptr[v + 1] - g.ptr[v];
    if (du <= 2 && dv <= 2) return -1;
    const int32_t ku = g.cid[u], kv = g.cid[v];
    if (ku < 0 || kv < 0) return GC_UNPL;
    const uint32_t d = (uint32_t)o.directionT & 3u, dr = (uint32_t)o.direction & 3u;      // the steps u -> v and v -> u
    const uint32_t urev = d >> 1, vrev = 1u - (d & 1u);
    const uint32_t bu = g.bits[u], bv = g.bits[v];
    const uint32_t su = (bu >> 2) & 1u, sv = (bv >> 2) & 1u;
    uint32_t frev, trev;
    if ((bu & GL_LAST) && urev == su) frev = 0;
    else if ((bu & GL_FIRST) && urev != su) frev = 1;
    else return GC_TWIST;
    if ((bv & GL_FIRST) && vrev == sv) trev = 0;
    else if ((bv & GL_LAST) && vrev != sv) trev = 1;
    else return GC_TWIST;
    const int64_t a = (int64_t)g.len[u] - o.suffix, b = (int64_t)g.len[v] - o.suffixT;
    const int64_t lu = g.soff[ku + 1] - g.soff[ku], lv = g.soff[kv + 1] - g.soff[kv];
    int64_t cap = lu < lv ? lu : lv;
    if (cap > 0x7fffffffll) cap = 0x7fffffffll;
    const int64_t raw = a < b ? a : b;
    const int64_t ov = raw < 0 ? 0 : raw > cap ? cap : raw;
    *clamped = ov != raw;
    *asym = dr != (((d & 1u) << 1) | (d >> 1));
    rec->from = (uint32_t)ku; rec->to = (uint32_t)kv; rec->from_read = u + g.base; rec->to_read = v + g.base;
    rec->overlap = (int32_t)ov; rec->from_rev = (uint8_t)frev; rec->to_rev = (uint8_t)trev; rec->flags = 0; rec->reserved = 0;
    return GC_LINKS;
}

__device__ __forceinline__ unsigned long long gl_wave_sum(unsigned long long v)
{
    for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s);
    return v;
}

// part: GC_PART words per workgroup, the count pass's counters (no atomics: every wavefront of a million-read graph adding to the same
// seven words cost more than the pass itself); k_gl_sum adds them up
constexpr int GC_PART = 8;
template <int EMIT>
__global__ __launch_bounds__(GL_THREADS) void k_gl_links(GlIn g, uint32_t *cnt, const uint32_t *off, elba_link_t *out, unsigned long long *part)
{
    __shared__ unsigned long long lsum[GL_THREADS / 64][GC_PART];
    const unsigned lane = threadIdx.x & 63;
    const uint32_t u0 = (blockIdx.x * GL_THREADS + threadIdx.x) & ~63u;      // the wavefront's first column
    const uint32_t u = u0 + lane;
    unsigned long long n[GC_N] = {0, 0, 0, 0, 0, 0, 0};
    uint32_t s = 0, du = 0, mine = 0, at = 0;
    bool is_long = false;
    if (u < g.M) {
        s = g.ptr[u]; du = g.ptr[u + 1] - s;
        if (EMIT) at = off[u];
        const int32_t k = g.cid[u];
        if (k >= 0 && (g.bits[u] & GL_FIRST) && g.kind[k] == 1) {             // the closure of a circular contig, at (u, u)
            if (EMIT) out[at] = elba_link_t{(uint32_t)k, (uint32_t)k, u + g.base, u + g.base, 0, 0, 0, 1, 0};
            ++mine; ++n[GC_CLOS];
        }
        is_long = du > GL_LANE_MAX;
        if (!is_long)
            for (uint32_t t = 0; t < du; ++t) {
                const int64_t r = g.rows[s + t];
                if (r <= (int64_t)u || r >= (int64_t)g.M) continue;
                elba_link_t rec; bool cl = false, as = false;
                const int what = gl_classify(g, u, du, (uint32_t)r, g.vals[s + t], &rec, &cl, &as);
                if (what < 0) continue;
                ++n[GC_CAND]; ++n[what];
                if (what == GC_LINKS) {
                    n[GC_CLAMP] += cl; n[GC_ASYM] += as;
                    if (EMIT) out[at + mine] = rec;
                    ++mine;
                }
            }
    }
    unsigned long long todo = __ballot(is_long);
    while (todo) {                                                             // uniform: every lane of the wavefront takes part
        const int src = __builtin_ctzll(todo);
        todo &= todo - 1;
        const uint32_t cu = u0 + (uint32_t)src;                                // < M: its lane said so
        const uint32_t cs = __shfl(s, src), cd = __shfl(du, src);
        uint32_t place = __shfl(mine, src);                                    // behind its closure record, if any
        const uint32_t cat = EMIT ? __shfl(at, src) : 0u;
        for (uint32_t t0 = 0; t0 < cd; t0 += 64) {
            const uint32_t t = t0 + lane;
            int what = -1;
            elba_link_t rec; bool cl = false, as = false;
            if (t < cd) {
                const int64_t r = g.rows[cs + t];
                if (r > (int64_t)cu && r < (int64_t)g.M) what = gl_classify(g, cu, cd, (uint32_t)r, g.vals[cs + t], &rec, &cl, &as);
            }
            if (what >= 0) { ++n[GC_CAND]; ++n[what]; }
            const bool link = what == GC_LINKS;
            if (link) { n[GC_CLAMP] += cl; n[GC_ASYM] += as; }
            const unsigned long long b = __ballot(link);
            if (EMIT && link) out[cat + place + (uint32_t)__builtin_popcountll(b & ((1ull << lane) - 1))] = rec;
            place += (uint32_t)__builtin_popcountll(b);
        }
        if ((int)lane == src) mine = place;
    }
    if (!EMIT) {
        if (u < g.M) cnt[u] = mine;
        else if (u == g.M) cnt[u] = 0;
        for (int i = 0; i < GC_N; ++i) {
            const unsigned long long t = gl_wave_sum(n[i]);
            if (lane == 0) lsum[threadIdx.x >> 6][i] = t;
        }
        __syncthreads();
        if (threadIdx.x < GC_N) {
            unsigned long long t = 0;
            for (int w = 0; w < GL_THREADS / 64; ++w) t += lsum[w][threadIdx.x];
            part[(size_t)blockIdx.x * GC_PART + threadIdx.x] = t;
        }
    }
}

__global__ __launch_bounds__(GL_THREADS) void k_gl_sum(const unsigned long long *part, uint32_t nblocks, unsigned long long *ctr)
{
    __shared__ unsigned long long lsum[GL_THREADS / 64][GC_PART];
    unsigned long long n[GC_N] = {0, 0, 0, 0, 0, 0, 0};
    for (uint32_t b = threadIdx.x; b < nblocks; b += GL_THREADS)
        for (int i = 0; i < GC_N; ++i) n[i] += part[(size_t)b * GC_PART + i];
    for (int i = 0; i < GC_N; ++i) {
        const unsigned long long t = gl_wave_sum(n[i]);
        if ((threadIdx.x & 63) == 0) lsum[threadIdx.x >> 6][i] = t;
    }
    __syncthreads();
    if (threadIdx.x < GC_N) {
        unsigned long long t = 0;
        for (int w = 0; w < GL_THREADS / 64; ++w) t += lsum[w][threadIdx.x];
        ctr[threadIdx.x] = t;
    }
}

}  // namespace

void stage_export_assembly_links(Ctx &c, elba_links_t *out)
{
    ELBA_REQUIRE(has(c.v, P_S, P_CONTIGS), ELBA_ERR_STATE, "export_assembly_links: no contigs of the current string graph (call elba_generate_contigs)");
    const int64_t M = c.tr_M, nnz = c.tr_nnz, base = c.tr_id_base, E = c.cg.E, nc = c.cg.n;
    const ReadSource src = read_source(c, M, "export_assembly_links", "lengths of the graph's # reads", base == 0);
    ELBA_REQUIRE(M + base < 0xFFFFFFFFll && nc < 0xFFFFFFFFll, ELBA_ERR_UNSUPPORTED, "export_assembly_links: read ids beyond 32 bit");
    hipStream_t s = c.stream;
    c.gl.ptr.reserve((size_t)(M + 2) * 4); c.gl.bits.reserve((size_t)M + 4); c.gl.cnt.reserve((size_t)(M + 2) * 4); c.gl.off.reserve((size_t)(M + 2) * 4);
    c.gl.ctr.reserve(64);
    const unsigned nb = (unsigned)((M + 1 + GL_THREADS - 1) / GL_THREADS);      // (column M: the scan's last element)
    c.gl.part.reserve((size_t)nb * GC_PART * 8);
    uint32_t *ptr = c.gl.ptr.as<uint32_t>(), *cnt = c.gl.cnt.as<uint32_t>(), *off = c.gl.off.as<uint32_t>();
    unsigned long long *ctr = c.gl.ctr.as<unsigned long long>();
    c.gl.t_total.start(s);
    ELBA_HIP(hipMemsetAsync(ctr, 0, 64, s));
    ELBA_HIP(hipMemsetAsync(c.gl.bits.p, 0, (size_t)M + 4, s));
    if (nnz > 0) group_offsets_u32(s, reinterpret_cast<const uint64_t *>(c.tr_out_cols.p), 0, nnz, ptr, M);     // column pointers of S (columns ascending)
    else ELBA_HIP(hipMemsetAsync(ptr, 0, (size_t)(M + 1) * 4, s));
    if (E > 0)
        hipLaunchKernelGGL(k_gl_bits, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, s, c.cg.eread.as<int64_t>(), c.cg.estr.as<uint8_t>(), c.cg.coff.as<int64_t>(),
                           c.cg.cid.as<int32_t>(), E, base, (uint32_t)M, c.gl.bits.as<uint8_t>());
    GlIn g{ptr, c.tr_out_rows.as<int64_t>(), c.tr_out_vals.as<elba_overlap_t>(), c.cg.cid.as<int32_t>(), c.gl.bits.as<uint8_t>(), c.cg.kind.as<uint8_t>(),
           c.cg.soff.as<int64_t>(), src.len, (uint32_t)M, (uint32_t)base};
    hipLaunchKernelGGL(k_gl_links<0>, dim3(nb), dim3(GL_THREADS), 0, s, g, cnt, (const uint32_t *)nullptr, (elba_link_t *)nullptr, c.gl.part.as<unsigned long long>());
    hipLaunchKernelGGL(k_gl_sum, dim3(1), dim3(GL_THREADS), 0, s, c.gl.part.as<unsigned long long>(), nb, ctr);
    exclusive_scan_u32(s, cnt, off, M + 1, c.ws_scan);
    ELBA_HIP(hipGetLastError());
    unsigned long long h[8] = {0};
    uint32_t total = 0;
    ELBA_HIP(hipMemcpyAsync(h, ctr, 64, hipMemcpyDeviceToHost, s));
    ELBA_HIP(hipMemcpyAsync(&total, off + M, 4, hipMemcpyDeviceToHost, s));
    ELBA_HIP(hipStreamSynchronize(s));
    ELBA_REQUIRE((unsigned long long)total == h[GC_LINKS] + h[GC_CLOS], ELBA_ERR_INTERNAL, "export_assembly_links: the scanned total is not the counted records");
    out->n = (int64_t)total;
    out->links = host_block<elba_link_t>((size_t)total);
    if (total) {
        c.gl.out.reserve((size_t)total * sizeof(elba_link_t));
        hipLaunchKernelGGL(k_gl_links<1>, dim3(nb), dim3(GL_THREADS), 0, s, g, cnt, (const uint32_t *)off, c.gl.out.as<elba_link_t>(), (unsigned long long *)nullptr);
        ELBA_HIP(hipGetLastError());
        copy_out(c, out->links, c.gl.out.p, (size_t)total);
    }
    c.gl.t_total.stop(s);
    ELBA_HIP(hipStreamSynchronize(s));
    elba_graph_stats st{};
    st.segments = nc; st.candidates = (int64_t)h[GC_CAND]; st.links = (int64_t)h[GC_LINKS]; st.closures = (int64_t)h[GC_CLOS]; st.twisted = (int64_t)h[GC_TWIST];
    st.unplaced = (int64_t)h[GC_UNPL]; st.clamped = (int64_t)h[GC_CLAMP]; st.asymmetric = (int64_t)h[GC_ASYM];
    st.ms_total = c.gl.t_total.ms();
    c.gl.stats = st; c.gl.for_cg = c.cg.serial;
}

}  // namespace elba
