// place.hip — every read on its contig, and the depth of every contig base (elba_place_reads; the rule is stated in include/elba_amd.h).
// The contig stage places the reads of its chains; everything the graph lost on the way — contained reads, reads a cleaning call removed,
// branches, reads whose edges the reduction dropped — is placed here through ONE aligned pair with a chain read, the best-scoring one.
//
// Input, all resident: of the last contig call the read map cg.cid, the chain arrays cg.eread / cg.estr / cg.eboff, the offsets cg.soff /
// cg.coff and the kinds; the read flags of the reduction and the cleaning calls (tr_flags); the read lengths; and the pairs the graph was
// built from (graph_input: the loaded edge list, else the context's alignments), which the reduction read and left as they were.
//
// The launches up to and including k_pl_place are place_records(), which elba_polish_contigs (polish.hip) calls for the same records.
//
//   k_pl_chain       one lane per chain element: start (its base offset minus its contig's) and strand of its read; one lane per contig:
//                    its length as u32 (the `len` of the segment passes)
//   k_pl_candidates  one lane per pair: passed, exactly one of its reads on a chain, the other without a skip bit and not empty -> a
//                    candidate; its two intervals are checked (0 <= beg <= end <= len: the smallest bad pair fails the call) and
//                    max(score, 0) << 32 | ~index goes into the off-chain read's word with one 64-bit atomicMax: the largest score wins, on
//                    a tie the smallest index, whatever the order.  The candidate count: one atomic per wavefront of a grid that only
//                    fills the device (16 workgroups per CU, lanes stride over the list).  With a wavefront per 64 pairs the count was
//                    one atomic on the same word per 64 pairs: 693 of the call's 945 us on dense-repeats-25th (4.15 M pairs)
//   k_pl_place       one lane per read: chain reads copy their start; the others decode the winner and apply the transform; the record (24
//                    bytes) and its clipped / outside / wrapped bits; the counts, one atomic per wavefront and counter
//   k_pl_emit        one lane per read: the one or two credited intervals of a placed read as endpoint keys contig << (pb + 1) | pos << 1 |
//                    kind (1 = start), in slot pairs drawn per wavefront with one atomic; the credited bases summed per wavefront; a wrapped
//                    read, whose two intervals would count it twice below, takes 1 off its contig's read count (an integer atomic: exact)
//   -- the one host synchronisation: the endpoint count E (and the bounds check) --
//   depth_segments   pileup.hip's sequence on the buffers of c.pl.depth with the contig lengths as `len`: radix sort of the E keys, group offsets,
//                    k_pu_marks, two scans, k_pu_groups, k_pu_tokens, scan, k_pu_segs
//   k_pl_credit      one lane per sorted key: start keys count 1 read and -pos bases, end keys +pos; a segmented scan over the wavefront by
//                    contig (the keys are sorted, a contig's keys are consecutive), the last lane of every run adds the run's two sums to
//                    its contig with integer atomics: credited_reads, credited_bases
//
// Bounds: pair reads are used only below M; a pair index decoded from a word was written by its lane, so it is below n; cid is read for
// reads below M and is below the contig count nc (soff has nc + 1 entries, clen / kind / cred nc); chain elements below E name reads below
// M; endpoint slots are 2 x (interval slot) with at most two intervals per read, so below 4M, which sizes the key buffers; keys carry
// contig < nc < 2^mb and pos <= length < 2^pb <= 2^31; the segment passes' own bounds are pileup.hip's with (4M, nc) for (4n, M).
// Bytes moved (algorithmic): 16 + 36 bytes per pair read, 1 + 4 + 4 bytes per pair read looked up, 8 bytes per candidate (atomic), 17 bytes
// per chain element, 24 bytes per read written and read again, 36 bytes per anchored read for its pair, 8 bytes per endpoint written, read +
// written per sort pass (8-bit digits over mb + pb + 1 bits), about 14 x 4 bytes per endpoint for the marks / scans / groups / tokens, 8
// bytes per endpoint for the credits, 8 bytes per segment written.
#include "common.hpp"

namespace elba {

namespace {

// counters: 0 candidates, 1 credited intervals, 2 smallest bad pair, 3 segments, 4 max depth (3 and 4: depth_segments), 5 chain, 6 anchored,
// 7 unanchored, 8 skipped, 9 empty, 10 clipped, 11 outside, 12 wrapped, 13 credited bases
enum { PC_CAND = 0, PC_INT, PC_BAD, PC_SEGS, PC_DEPTH, PC_CHAIN, PC_ANCH, PC_UNANCH, PC_SKIP, PC_EMPTY, PC_CLIP, PC_OUT, PC_WRAP, PC_BASES, PC_N = 16 };
enum { PL_CLIPPED = 1, PL_OUTSIDE = 2, PL_WRAPPED = 4 };

struct PlIn {
    const int64_t *rows, *cols; const elba_overlap_t *vals; int64_t n;      // the graph's input pairs
    const int32_t *cid; const uint8_t *rflags; const uint32_t *len;         // per read: contig (-1: none), flags, length
    const int64_t *cstart; const uint8_t *cstrand;                          // per chain read: start and strand on its contig
    const uint32_t *clen; const uint8_t *kind;                              // per contig
    uint32_t M, base; int skip;
};

__device__ __forceinline__ unsigned long long pl_wave_count(bool b) { return (unsigned long long)__builtin_popcountll(__ballot(b)); }

// the credited intervals [lo[0], hi[0]) and, wrapped, [lo[1], hi[1]) of a read of l bases at `start` on a contig of L bases; returns the flag bits
__device__ __forceinline__ uint32_t pl_credit(int64_t start, int64_t l, int64_t L, uint32_t kind, int64_t lo[2], int64_t hi[2], int *nint)
{
    uint32_t f = 0;
    *nint = 0;
    if (kind == 1) {                                            // circular
        const int64_t cred = l < L ? l : L;
        if (l > L) f |= PL_CLIPPED;
        if (cred <= 0) return f | PL_OUTSIDE;
        int64_t m = start % L;
        if (m < 0) m += L;
        if (m + cred > L) { lo[0] = m; hi[0] = L; lo[1] = 0; hi[1] = m + cred - L; *nint = 2; f |= PL_WRAPPED; }
        else { lo[0] = m; hi[0] = m + cred; *nint = 1; }
        return f;
    }
    const int64_t a = start < 0 ? 0 : start, b = start + l < L ? start + l : L;
    if (a != start || b != start + l) f |= PL_CLIPPED;
    if (b <= a) return f | PL_OUTSIDE;
    lo[0] = a; hi[0] = b; *nint = 1;
    return f;
}

__global__ void k_pl_chain(const int64_t *eread, const uint8_t *estr, const int64_t *eboff, const int32_t *cid, const int64_t *soff, int64_t E, int64_t nc,
                           int64_t base, uint32_t M, int64_t *cstart, uint8_t *cstrand, uint32_t *clen)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < nc) clen[e] = (uint32_t)(soff[e + 1] - soff[e]);
    if (e >= E) return;
    const int64_t r = eread[e] - base;
    if (r < 0 || r >= (int64_t)M) return;
    const int32_t k = cid[r];
    if (k < 0) return;
    cstart[r] = eboff[e] - soff[k]; cstrand[r] = estr[e];
}

__global__ void k_pl_candidates(PlIn g, unsigned long long *best, unsigned long long *ctr)
{
    unsigned long long mine = 0;                                // this lane's candidates, over all its trips
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; a < g.n; a += stride) {
        const elba_overlap_t o = g.vals[a];
        const uint64_t q = (uint64_t)g.rows[a], t = (uint64_t)g.cols[a];
        if (o.passed == 0 || q >= g.M || t >= g.M) continue;
        const bool qc = g.cid[q] >= 0, tc = g.cid[t] >= 0;
        if (qc == tc) continue;
        const uint32_t x = (uint32_t)(qc ? t : q);
        if ((g.rflags[x] & g.skip) || g.len[x] == 0) continue;
        ++mine;
        const int64_t lq = g.len[q], lt = g.len[t];
        const bool ok = o.begQ >= 0 && o.begQ <= o.endQ && o.endQ <= lq && o.begT >= 0 && o.begT <= o.endT && o.endT <= lt;
        if (!ok) atomicMin(&ctr[PC_BAD], (unsigned long long)a);
        else atomicMax(&best[x], ((unsigned long long)(o.score > 0 ? o.score : 0) << 32) | (uint32_t)~(uint32_t)a);
    }
    for (int o = 32; o >= 1; o >>= 1) mine += (unsigned long long)__shfl_xor((long long)mine, o);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&ctr[PC_CAND], mine);
}

__global__ void k_pl_place(PlIn g, const unsigned long long *best, elba_placement_t *rec, unsigned long long *ctr)
{
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    int what = -1;                                              // the counter of this read
    uint32_t f = 0;
    if (r < g.M) {
        elba_placement_t p{0, -1, r + g.base, 0, 0, 0, 0, 0};
        const int32_t k = g.cid[r];
        if (k >= 0) { p.start = g.cstart[r]; p.contig = k; p.strand = g.cstrand[r]; p.kind = 1; what = PC_CHAIN; }
        else if (g.rflags[r] & g.skip) what = PC_SKIP;
        else if (g.len[r] == 0) what = PC_EMPTY;
        else {
            const unsigned long long w = best[r];
            if (!w) what = PC_UNANCH;
            else {
                const uint32_t a = ~(uint32_t)w;
                const elba_overlap_t o = g.vals[a];
                const bool xq = (uint32_t)g.rows[a] == r;                     // r is the pair's Q, the chain read its T — or the other way round
                const uint32_t y = (uint32_t)(xq ? g.cols[a] : g.rows[a]);
                const int64_t lx = g.len[r], ly = g.len[y];
                const int64_t bx = xq ? o.begQ : o.begT, ex = xq ? o.endQ : o.endT, by = xq ? o.begT : o.begQ, ey = xq ? o.endT : o.endQ;
                const uint32_t sy = g.cstrand[y] ? 1u : 0u, sx = sy ^ (o.rc ? 1u : 0u);
                const int64_t oby = sy ? ly - ey : by, obx = sx ? lx - ex : bx;
                p.start = g.cstart[y] + oby - obx; p.contig = g.cid[y]; p.anchor = y + g.base; p.score = o.score; p.strand = (uint8_t)sx; p.kind = 2;
                what = PC_ANCH;
            }
        }
        if (p.kind) {
            int64_t lo[2], hi[2]; int nint;
            f = pl_credit(p.start, g.len[r], g.clen[p.contig], g.kind[p.contig], lo, hi, &nint);
            p.flags = (uint8_t)f;
        }
        rec[r] = p;
    }
    const unsigned lane = threadIdx.x & 63;
    for (int i = PC_CHAIN; i <= PC_EMPTY; ++i) {
        const unsigned long long n = pl_wave_count(what == i);
        if (lane == 0 && n) atomicAdd(&ctr[i], n);
    }
    const unsigned long long ncl = pl_wave_count(f & PL_CLIPPED), no = pl_wave_count(f & PL_OUTSIDE), nw = pl_wave_count(f & PL_WRAPPED);
    if (lane == 0) {
        if (ncl) atomicAdd(&ctr[PC_CLIP], ncl);
        if (no) atomicAdd(&ctr[PC_OUT], no);
        if (nw) atomicAdd(&ctr[PC_WRAP], nw);
    }
}

__global__ void k_pl_emit(const elba_placement_t *rec, const uint32_t *len, const uint32_t *clen, const uint8_t *kind, uint32_t M, int pb, uint64_t *keys,
                          unsigned long long *cred_reads, unsigned long long *ctr)
{
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    int64_t lo[2] = {0, 0}, hi[2] = {0, 0};
    int nint = 0;
    uint64_t cbits = 0;
    if (r < M) {
        const elba_placement_t p = rec[r];
        if (p.kind) {
            pl_credit(p.start, len[r], clen[p.contig], kind[p.contig], lo, hi, &nint);
            cbits = (uint64_t)(uint32_t)p.contig << (pb + 1);
            if (nint == 2) atomicAdd(&cred_reads[p.contig], ~0ull);            // (-1: its two intervals are one read)
        }
    }
    // the wave's credited intervals take consecutive slot pairs from one atomic on the interval counter (the sort restores an order)
    const unsigned lane = threadIdx.x & 63;
    const unsigned long long b1 = __ballot(nint >= 1), b2 = __ballot(nint == 2);
    const unsigned n = (unsigned)(__builtin_popcountll(b1) + __builtin_popcountll(b2));
    unsigned long long bases = (unsigned long long)((hi[0] - lo[0]) + (hi[1] - lo[1]));
    for (int o = 32; o >= 1; o >>= 1) bases += (unsigned long long)__shfl_xor((long long)bases, o);
    unsigned long long slot = 0;
    if (lane == 0) {
        if (n) slot = atomicAdd(&ctr[PC_INT], (unsigned long long)n);
        if (bases) atomicAdd(&ctr[PC_BASES], bases);
    }
    slot = __shfl(slot, 0);
    const unsigned long long below = (1ull << lane) - 1;
    uint64_t *dst = keys + 2 * (slot + __builtin_popcountll(b1 & below) + __builtin_popcountll(b2 & below));
    for (int i = 0; i < nint; ++i, dst += 2) { dst[0] = cbits | ((uint64_t)lo[i] << 1) | 1u; dst[1] = cbits | ((uint64_t)hi[i] << 1); }
}

__global__ void k_pl_credit(const uint64_t *keys, int64_t E, int pb, unsigned long long *cred_reads, unsigned long long *cred_bases)
{
    const int64_t z = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned lane = threadIdx.x & 63;
    unsigned long long c = ~0ull, vr = 0;
    long long vb = 0;
    if (z < E) {
        const uint64_t k = keys[z];
        const long long pos = (long long)((k >> 1) & ((1ull << pb) - 1));
        c = k >> (pb + 1); vr = k & 1u; vb = (k & 1u) ? -pos : pos;
    }
    for (unsigned o = 1; o < 64; o <<= 1) {                     // a run of equal contigs is consecutive: the partial sums never leave it
        const unsigned long long co = __shfl_up(c, o), ro = __shfl_up(vr, o);
        const long long bo = __shfl_up(vb, o);
        if (lane >= o && co == c) { vr += ro; vb += bo; }
    }
    const unsigned long long cn = __shfl_down(c, 1);
    if (z < E && (lane == 63 || cn != c)) {                     // the last key of its contig in this wavefront (sums are modulo 2^64: a run may end negative)
        if (vr) atomicAdd(&cred_reads[c], vr);
        if (vb) atomicAdd(&cred_bases[c], (unsigned long long)vb);
    }
}

}  // namespace

static_assert(PC_BAD == PLACE_CTR_BAD && PC_N == PLACE_CTR_WORDS, "common.hpp names the counters of place_records");

PlaceWork place_records(Ctx &c, int skip_flags, const char *who_, bool depth_bufs, EventTimer *t)
{
    const std::string who(who_);
    ELBA_REQUIRE(has(c.v, P_S, P_CONTIGS), ELBA_ERR_STATE, who + ": no contigs of the current string graph (call elba_generate_contigs)");
    const GraphInput in = graph_input(c, who_);
    const int64_t M = c.tr_M, base = c.tr_id_base, E = c.cg.E, nc = c.cg.n, n = in.n;
    ELBA_REQUIRE(in.M == M && in.id_base == base, ELBA_ERR_STATE, who + ": the pairs on this context are not the ones the string graph was built from");
    const ReadSource src = read_source(c, M, who_, "lengths of the graph's # reads", base == 0);
    ELBA_REQUIRE(M + base < 0xFFFFFFFFll && n < 0xFFFFFFFFll, ELBA_ERR_UNSUPPORTED, who + ": read ids or pairs beyond 32 bit");
    ELBA_REQUIRE(c.cg.stats.longest < (1ll << 31), ELBA_ERR_UNSUPPORTED, who + ": a contig of 2^31 bases or more");
    ELBA_REQUIRE(4 * M + nc < 0xfffffff0ll, ELBA_ERR_UNSUPPORTED, who + ": 4 x reads + contigs reach 2^32");
    hipStream_t s = c.stream;
    if (depth_bufs) c.pl.depth.reserve(4 * M, nc);              // at most two intervals of two endpoints per read
    c.pl.cstart.reserve((size_t)(M + 1) * 8); c.pl.cstrand.reserve((size_t)M + 4); c.pl.best.reserve((size_t)(M + 1) * 8);
    c.pl.rec.reserve((size_t)(M + 1) * sizeof(elba_placement_t)); c.pl.clen.reserve((size_t)(nc + 1) * 4); c.pl.cred.reserve((size_t)(2 * nc + 2) * 8);
    c.pl.ctr.reserve(PC_N * 8);
    unsigned long long *ctr = c.pl.ctr.as<unsigned long long>(), *best = c.pl.best.as<unsigned long long>();
    elba_placement_t *rec = c.pl.rec.as<elba_placement_t>();
    PlIn g{in.rows, in.cols, in.vals, n, c.cg.cid.as<int32_t>(), c.tr_flags.as<uint8_t>(), src.len, c.pl.cstart.as<int64_t>(), c.pl.cstrand.as<uint8_t>(),
           c.pl.clen.as<uint32_t>(), c.cg.kind.as<uint8_t>(), (uint32_t)M, (uint32_t)base, skip_flags};
    if (t) t->start(s);
    ELBA_HIP(hipMemsetAsync(ctr, 0, PC_N * 8, s));
    ELBA_HIP(hipMemsetAsync(ctr + PC_BAD, 0xff, 8, s));
    ELBA_HIP(hipMemsetAsync(best, 0, (size_t)(M + 1) * 8, s));
    ELBA_HIP(hipMemsetAsync(c.pl.cred.p, 0, (size_t)(2 * nc + 2) * 8, s));
    const int64_t nce = E > nc ? E : nc;
    if (nce > 0)
        hipLaunchKernelGGL(k_pl_chain, dim3((unsigned)((nce + 255) / 256)), dim3(256), 0, s, c.cg.eread.as<int64_t>(), c.cg.estr.as<uint8_t>(), c.cg.eboff.as<int64_t>(),
                           c.cg.cid.as<int32_t>(), c.cg.soff.as<int64_t>(), E, nc, base, (uint32_t)M, c.pl.cstart.as<int64_t>(), c.pl.cstrand.as<uint8_t>(), c.pl.clen.as<uint32_t>());
    if (n > 0) {                                                // (a grid that fills the device, every lane striding over the list: see the header)
        int64_t grid = (n + 255) / 256;
        if (grid > (int64_t)c.num_cus * 16) grid = (int64_t)c.num_cus * 16;
        hipLaunchKernelGGL(k_pl_candidates, dim3((unsigned)grid), dim3(256), 0, s, g, best, ctr);
    }
    if (M > 0) hipLaunchKernelGGL(k_pl_place, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, g, (const unsigned long long *)best, rec, ctr);
    return PlaceWork{in, src, M, base, E, nc, rec, ctr, c.pl.clen.as<uint32_t>()};
}

void stage_place_reads(Ctx &c, const elba_place_cfg *cfg, elba_placements_t *out)
{
    c.pl.for_cg = 0;                                               // (whatever this call ends in, the counts of the one before are gone)
    ELBA_REQUIRE(cfg, ELBA_ERR_INVALID_ARG, "place_reads: null cfg");
    ELBA_REQUIRE(!cfg->reserved[0] && !cfg->reserved[1] && !cfg->reserved[2], ELBA_ERR_INVALID_ARG, "place_reads: reserved words must be 0");
    ELBA_REQUIRE(cfg->skip_flags >= 0 && cfg->skip_flags <= 255, ELBA_ERR_INVALID_ARG, "place_reads: skip_flags must fit in one byte");
    const PlaceWork w = place_records(c, cfg->skip_flags, "place_reads", true, &c.pl.t_total);
    const ReadSource &src = w.src;
    const int64_t M = w.M, nc = w.nc;
    hipStream_t s = c.stream;
    int mb = 1, pb = 1;
    while ((1ll << mb) < nc + 1) ++mb;
    while ((1ll << pb) < c.cg.stats.longest + 1) ++pb;            // positions 0 .. length
    DepthBufs &db = c.pl.depth;
    unsigned long long *ctr = w.ctr;
    unsigned long long *cred_reads = c.pl.cred.as<unsigned long long>(), *cred_bases = cred_reads + nc;
    elba_placement_t *rec = w.rec;
    if (M > 0)
        hipLaunchKernelGGL(k_pl_emit, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, (const elba_placement_t *)rec, src.len, c.pl.clen.as<uint32_t>(), c.cg.kind.as<uint8_t>(), (uint32_t)M, pb,
                           db.k0.as<uint64_t>(), cred_reads, ctr);
    ELBA_HIP(hipGetLastError());
    unsigned long long h[PC_N] = {0};
    ELBA_HIP(hipMemcpyAsync(h, ctr, PC_N * 8, hipMemcpyDeviceToHost, s));
    ELBA_HIP(hipStreamSynchronize(s));
    if (h[PC_BAD] != ~0ull) throw_bad_pair(c, w.in, (int64_t)h[PC_BAD], "place_reads");
    const int64_t K = 2 * (int64_t)h[PC_INT];                   // endpoints
    ELBA_REQUIRE(K <= 4 * M, ELBA_ERR_INTERNAL, "place_reads: more endpoints than four per read");
    const uint64_t *keys = depth_segments(c, db, K, nc, mb, pb, c.pl.clen.as<uint32_t>(), ctr);
    if (K > 0) hipLaunchKernelGGL(k_pl_credit, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, s, keys, K, pb, cred_reads, cred_bases);
    ELBA_HIP(hipGetLastError());
    c.pl.t_total.stop(s);
    // the segments are at most one per endpoint and one per contig: the copies are queued at that size, the count comes back with them
    const int64_t segcap = K + nc;
    elba_placements_t &o = *out;                                // (zeroed by the caller; every block lands in it at once, so that elba_free_placements releases what a failed allocation or copy leaves)
    o.nreads = M; o.ncontigs = nc;
    o.reads = host_block<elba_placement_t>((size_t)M); o.seg_off = host_block<int64_t>((size_t)nc + 1);
    o.seg_start = host_block<int32_t>((size_t)segcap); o.seg_depth = host_block<int32_t>((size_t)segcap);
    o.credited_reads = host_block<int64_t>((size_t)nc); o.credited_bases = host_block<int64_t>((size_t)nc);
    copy_out(c, o.reads, rec, (size_t)M);
    copy_out(c, o.seg_off, db.seg_off.p, (size_t)nc + 1);
    copy_out(c, o.seg_start, db.seg_start.p, (size_t)segcap); copy_out(c, o.seg_depth, db.seg_depth.p, (size_t)segcap);
    copy_out(c, o.credited_reads, cred_reads, (size_t)nc); copy_out(c, o.credited_bases, cred_bases, (size_t)nc);
    ELBA_HIP(hipMemcpyAsync(h, ctr, PC_N * 8, hipMemcpyDeviceToHost, s));
    ELBA_HIP(hipStreamSynchronize(s));
    ELBA_REQUIRE((int64_t)h[PC_SEGS] <= segcap && o.seg_off[nc] == (int64_t)h[PC_SEGS], ELBA_ERR_INTERNAL, "place_reads: the segment offsets do not end at the segment count");
    elba_place_stats st{};
    st.nreads = M; st.chain = (int64_t)h[PC_CHAIN]; st.anchored = (int64_t)h[PC_ANCH]; st.unanchored = (int64_t)h[PC_UNANCH]; st.skipped = (int64_t)h[PC_SKIP];
    st.empty = (int64_t)h[PC_EMPTY]; st.candidates = (int64_t)h[PC_CAND]; st.clipped = (int64_t)h[PC_CLIP]; st.outside = (int64_t)h[PC_OUT]; st.wrapped = (int64_t)h[PC_WRAP];
    st.segments = (int64_t)h[PC_SEGS]; st.max_depth = (int64_t)h[PC_DEPTH]; st.credited_bases = (int64_t)h[PC_BASES];
    st.ms_total = c.pl.t_total.ms();
    c.pl.stats = st; c.pl.for_cg = c.cg.serial;
}

}  // namespace elba
