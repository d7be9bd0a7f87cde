// pileup.hip — per-read coverage pileups, trimmed intervals and chimera flags from the aligned pairs: what PileupVector / GetReadPileup /
// GetTrimmedInterval (src/PruneChimeras.cpp:14-69,108-158, include/PruneChimeras.hpp) set out to compute, and R->PruneFull(x, x) of the
// reads it flags.  main.cpp never calls that file; here it sits between elba_align_seeds and elba_transitive_reduction.
//
// Input: the pairs the next elba_transitive_reduction would read (the list of elba_set_overlaps, else this context's alignments).  Each
// accepted pair (q, t) credits [beg + margin, end - margin) of BOTH reads (GetReadPileup credits only the column read of the upper-triangular
// R, :137-146 — a read gets coverage from its smaller-id partners only; here R + R^T).  begT / endT are on T's forward strand also when rc
// is set (xdrop_aligner maps them back, src/XDropAligner.cpp:275-276), so they are used as stored.
//
//   k_pu_emit      per pair: mode test, margin, bounds check (0 <= beg <= end <= len, :26), two endpoint keys per credited interval,
//                  read << (pb + 1) | pos << 1 | kind (kind 1 = start, +1; 0 = end, -1), compacted: one atomic per wavefront
//   -- the one host synchronisation: the endpoint count E (and the bounds check) --
//   radix sort     of the E keys on bits [0, mb + pb + 1): reads ascending, positions ascending inside a read (the degree skew of
//                  repeat-rich reads costs nothing extra: no per-read tile, no fall-back)
//   offsets        eptr[r] = first endpoint of read r (group_offsets on the read bits); eptr[M] = endpoints E
//   k_pu_marks     head = first endpoint of a (read, pos) group; delta = +1 / -1 as u32 (wraps, see below)
//   scans          group index of every head; prefix sums of the deltas.  A read's deltas sum to 0, so the global prefix sum at the end of
//                  a group IS the depth of its read right after that position (values inside a group may wrap: never read)
//   k_pu_groups    gstart[g] = first endpoint of group g
//   k_pu_tokens    one token per read (its leading (0, 0) segment) and per group: read r's token sits at gptr[r] + r, group g's at g + r + 1.
//                  A group emits (pos, depth after) when the depth changes and pos < len; the leading (0, 0) is emitted when len > 0 and no
//                  group opens a segment at 0
//   scan           segment index of every emitted token (gaps of unused tokens are zero)
//   k_pu_segs      seg_start / seg_depth, seg_off[r] (i64); maximal runs of equal depth, starts from 0, the last one ends at len
//   k_pu_reads     one lane per read over its segments: runs of depth >= min_depth (flags bit 0: none of length >= min_run; bit 1: two or
//                  more), the trimmed interval by GetTrimmedInterval's rule (:31-61) base by base where it can change anything, stats
//
// GetTrimmedInterval computes beststart / bestend and returns the run still open at the last base (:68); here the best one is returned,
// half-open [beststart, bestend + 1), (-1, -1) when no run qualified.  Bases of a run whose span is <= maxlen cannot replace the best
// (span > maxlen is required) and are summed in closed form (integer sums: exact); from the first base with span > maxlen on, every base is
// evaluated as the reference does, curavg = (double)curbases / (double)span (correctly rounded: the same value the host computes).
//
// Bounds: keys carry read < M, pos <= len < 2^pb; endpoint slots < E = 2 x credited intervals <= 4n (the key buffer holds 4n);
// group_offsets writes eptr[0 .. M]; group ids < G <= E, token slots < G + M <= E + M, segment ids < the scan's total.  Bytes moved
// (algorithmic): 52 B per pair read, 8 B per endpoint written, read + written per sort pass (8-bit digits over mb + pb + 1 bits), about
// 14 x 4 B per endpoint for the marks / scans / groups / tokens, 8 B per segment written.
#include "common.hpp"

namespace elba {

namespace {

struct PuParams {
    const int64_t *rows, *cols; const elba_overlap_t *vals; int64_t n;
    const uint32_t *len; uint32_t M; int pb;
    int mode, margin, min_depth, min_run, trim_len;
    uint64_t *keys;
    unsigned long long *ctr;   // 0 pairs used, 1 intervals credited, 2 smallest bad pair, 3 segments, 4 max depth, 5 unsupported, 6 split, 7 trimmed, 8 trimmed bases
};

__device__ __forceinline__ unsigned long long wave_sum(bool b) { return (unsigned long long)__builtin_popcountll(__ballot(b)); }

__global__ void k_pu_emit(PuParams p)
{
    const int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool used = false, cq = false, ct = false;
    uint64_t k[4] = {0, 0, 0, 0};
    if (a < p.n) {
        const elba_overlap_t o = p.vals[a];
        used = p.mode == 0 ? o.passed != 0 : o.score > 0;
        if (used) {
            const uint32_t q = (uint32_t)p.rows[a], t = (uint32_t)p.cols[a];
            const int64_t lq = p.len[q], lt = p.len[t];
            const bool ok = o.begQ >= 0 && o.begQ <= o.endQ && o.endQ <= lq && o.begT >= 0 && o.begT <= o.endT && o.endT <= lt;
            if (!ok) { atomicMin(&p.ctr[2], (unsigned long long)a); used = false; }
            else {
                const int64_t bq = (int64_t)o.begQ + p.margin, eq = (int64_t)o.endQ - p.margin, bt = (int64_t)o.begT + p.margin, et = (int64_t)o.endT - p.margin;
                cq = bq < eq; ct = bt < et;
                k[0] = ((uint64_t)q << (p.pb + 1)) | ((uint64_t)bq << 1) | 1u; k[1] = ((uint64_t)q << (p.pb + 1)) | ((uint64_t)eq << 1);
                k[2] = ((uint64_t)t << (p.pb + 1)) | ((uint64_t)bt << 1) | 1u; k[3] = ((uint64_t)t << (p.pb + 1)) | ((uint64_t)et << 1);
            }
        }
    }
    // the wave's credited intervals take consecutive slot pairs from one atomic on the interval counter (the sort restores an order)
    const unsigned lane = threadIdx.x & 63;
    const unsigned long long bu = __ballot(used), bq = __ballot(cq), bt = __ballot(ct);
    const unsigned nint = (unsigned)(__builtin_popcountll(bq) + __builtin_popcountll(bt));
    unsigned long long base = 0;
    if (lane == 0) {
        if (bu) atomicAdd(&p.ctr[0], (unsigned long long)__builtin_popcountll(bu));
        if (nint) base = atomicAdd(&p.ctr[1], (unsigned long long)nint);
    }
    base = __shfl(base, 0);
    const unsigned long long below = (1ull << lane) - 1;
    uint64_t *dst = p.keys + 2 * (base + __builtin_popcountll(bq & below) + __builtin_popcountll(bt & below));
    if (cq) { dst[0] = k[0]; dst[1] = k[1]; dst += 2; }
    if (ct) { dst[0] = k[2]; dst[1] = k[3]; }
}

// head / delta of every endpoint z < E (E = eptr[M]); the closing slot E gets 0, 0
__global__ void k_pu_marks(const uint64_t *keys, const uint32_t *eptr, uint32_t M, int64_t nslots, uint32_t *head, uint32_t *delta)
{
    const int64_t z = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (z > nslots) return;
    const int64_t E = eptr[M];
    uint32_t h = 0, d = 0;
    if (z < E) {
        const uint64_t k = keys[z];
        h = (z == 0 || (keys[z - 1] >> 1) != (k >> 1)) ? 1u : 0u;
        d = (k & 1u) ? 1u : 0xffffffffu;
    }
    head[z] = h; delta[z] = d;
}

__global__ void k_pu_groups(const uint32_t *head, const uint32_t *hidx, const uint32_t *eptr, uint32_t M, int64_t nslots, uint32_t *gstart)
{
    const int64_t z = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (z > nslots) return;
    const int64_t E = eptr[M];
    if (z < E && head[z]) gstart[hidx[z]] = (uint32_t)z;
    else if (z == E) gstart[hidx[E]] = (uint32_t)E;             // closing entry: gstart[G] = E
}

__device__ __forceinline__ bool pu_group_emits(const uint64_t *keys, const uint32_t *gstart, const uint32_t *dsum, uint32_t g, int pb, const uint32_t *len,
                                               uint32_t *r_out, uint32_t *pos_out, uint32_t *depth_out)
{
    const uint32_t zf = gstart[g], zl1 = gstart[g + 1];
    const uint64_t k = keys[zf];
    const uint32_t r = (uint32_t)(k >> (pb + 1)), pos = (uint32_t)((k >> 1) & ((1ull << pb) - 1));
    const uint32_t before = dsum[zf], after = dsum[zl1];
    *r_out = r; *pos_out = pos; *depth_out = after;
    return pos < len[r] && after != before;
}

// tokens: group g of read r at g + r + 1, the leading segment of read r at gptr[r] + r (gptr[r] = hidx[eptr[r]]: groups of the reads before r)
__global__ void k_pu_tokens(const uint64_t *keys, const uint32_t *eptr, const uint32_t *hidx, const uint32_t *gstart, const uint32_t *dsum, const uint32_t *len,
                            uint32_t M, int pb, int64_t nslots, uint32_t *tok)
{
    const int64_t z = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t E = eptr[M], G = hidx[E];
    if (z < (int64_t)G) {
        uint32_t r, pos, depth;
        const bool e = pu_group_emits(keys, gstart, dsum, (uint32_t)z, pb, len, &r, &pos, &depth);
        tok[z + r + 1] = e ? 1u : 0u;
    }
    if (z < (int64_t)M) {
        const uint32_t r = (uint32_t)z, e0 = eptr[r], e1 = eptr[r + 1], g0 = hidx[e0];
        bool lead = len[r] > 0;
        if (lead && e0 < e1) {
            uint32_t rr, pos, depth;
            if (pu_group_emits(keys, gstart, dsum, g0, pb, len, &rr, &pos, &depth) && pos == 0) lead = false;
        }
        tok[g0 + r] = lead ? 1u : 0u;
    }
}

__global__ void k_pu_segs(const uint64_t *keys, const uint32_t *eptr, const uint32_t *hidx, const uint32_t *gstart, const uint32_t *dsum, const uint32_t *len,
                          const uint32_t *tok, const uint32_t *tpos, uint32_t M, int pb, int64_t ntok, int64_t *seg_off, int32_t *seg_start, int32_t *seg_depth,
                          unsigned long long *ctr)
{
    const int64_t z = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t E = eptr[M], G = hidx[E];
    uint32_t dmax = 0;
    if (z < (int64_t)G) {
        uint32_t r, pos, depth;
        if (pu_group_emits(keys, gstart, dsum, (uint32_t)z, pb, len, &r, &pos, &depth)) {
            const uint32_t at = tpos[z + r + 1];
            seg_start[at] = (int32_t)pos; seg_depth[at] = (int32_t)depth;
            dmax = depth;
        }
    }
    if (z < (int64_t)M) {
        const uint32_t r = (uint32_t)z, g0 = hidx[eptr[r]];
        const uint32_t at = tpos[g0 + r];
        seg_off[r] = at;
        if (tok[g0 + r]) { seg_start[at] = 0; seg_depth[at] = 0; }
    } else if (z == (int64_t)M) {
        const uint32_t total = tpos[ntok];
        seg_off[M] = total;
        ctr[3] = total;
    }
    // one atomic per wavefront: the wave's largest depth
    unsigned v = dmax;
    for (int o = 32; o >= 1; o >>= 1) { const unsigned w = (unsigned)__shfl_xor((int)v, o); v = w > v ? w : v; }
    if ((threadIdx.x & 63) == 0 && v) atomicMax(&ctr[4], (unsigned long long)v);
}

// one lane per read: runs of depth >= min_depth, flags, the trimmed interval (GetTrimmedInterval's rule, best run returned)
__global__ void k_pu_reads(const int64_t *seg_off, const int32_t *seg_start, const int32_t *seg_depth, const uint32_t *len, uint32_t M, int min_depth, int min_run,
                           int trim_len, int2 *trim, uint8_t *flags, unsigned long long *ctr)
{
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    bool unsupported = false, split = false, trimmed = false;
    unsigned long long tb = 0;
    if (r < M) {
        const int64_t s0 = seg_off[r], s1 = seg_off[r + 1];
        const int64_t L = len[r];
        int64_t maxlen = trim_len, beststart = -1, bestend = -1;
        double bestavg = 0.0;
        int64_t start = -1, curbases = 0;
        uint32_t long_runs = 0;
        for (int64_t j = s0; j < s1; ++j) {
            const int64_t a = seg_start[j], b = j + 1 < s1 ? seg_start[j + 1] : L;
            const int64_t d = seg_depth[j];
            if (d < min_depth) {
                if (start >= 0 && a - start >= min_run) ++long_runs;
                start = -1;
                continue;
            }
            if (start < 0) { start = a; curbases = 0; }
            // bases i in [a, b): span = i - start + 1; only bases with span > maxlen can replace the best
            int64_t i = start + maxlen;                              // first base with span = maxlen + 1
            if (i >= b) { curbases += d * (b - a); continue; }
            if (i < a) i = a;
            curbases += d * (i - a);
            for (; i < b; ++i) {
                curbases += d;
                const int64_t span = i - start + 1;
                const double curavg = (double)curbases / (double)span;
                if (span > maxlen && curavg > bestavg) { beststart = start; bestend = i; maxlen = span; bestavg = curavg; }
            }
        }
        if (start >= 0 && L - start >= min_run) ++long_runs;
        unsupported = long_runs == 0;
        split = long_runs >= 2;
        const int32_t tb0 = beststart < 0 ? -1 : (int32_t)beststart, te0 = beststart < 0 ? -1 : (int32_t)(bestend + 1);
        trim[r] = make_int2(tb0, te0);
        flags[r] = (uint8_t)((unsupported ? 1 : 0) | (split ? 2 : 0));
        trimmed = !(tb0 == 0 && te0 == L);
        if (tb0 >= 0) tb = (unsigned long long)(te0 - tb0);
    }
    const unsigned lane = threadIdx.x & 63;
    const unsigned long long nu = wave_sum(unsupported), ns = wave_sum(split), nt = wave_sum(trimmed);
    unsigned long long v = tb;
    for (int o = 32; o >= 1; o >>= 1) v += (unsigned long long)__shfl_xor((long long)v, o);
    if (lane == 0) {
        if (nu) atomicAdd(&ctr[5], nu);
        if (ns) atomicAdd(&ctr[6], ns);
        if (nt) atomicAdd(&ctr[7], nt);
        if (v) atomicAdd(&ctr[8], v);
    }
}

__global__ void k_pu_prune_select(const int64_t *rows, const int64_t *cols, int64_t n, const uint8_t *flags, uint8_t mask, uint32_t *sel)
{
    const int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (a < n) sel[a] = ((flags[rows[a]] | flags[cols[a]]) & mask) ? 0u : 1u;
    else if (a == n) sel[a] = 0u;
}

__global__ void k_pu_prune_scatter(const int64_t *rows, const int64_t *cols, const elba_overlap_t *vals, int64_t n, const uint32_t *sel, const uint32_t *pos,
                                   int64_t *orow, int64_t *ocol, elba_overlap_t *oval)
{
    const int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= n || !sel[a]) return;
    const uint32_t at = pos[a];
    orow[at] = rows[a]; ocol[at] = cols[a]; oval[at] = vals[a];
}

struct PuInput : GraphInput { const uint32_t *len; uint32_t maxlen; };

// the pairs elba_transitive_reduction would read next and the lengths of reads 0 .. M-1
PuInput pileup_input(Ctx &c, const char *who)
{
    PuInput in{graph_input(c, who), nullptr, 0};
    const ReadSource src = read_source(c, in.M, who, "lengths of the # reads of the overlaps");
    in.len = src.len;
    if (src.replicated) in.maxlen = c.aln_all_maxlen;
    else for (uint32_t l : c.h_len) in.maxlen = l > in.maxlen ? l : in.maxlen;
    return in;
}

}  // namespace

// Sorted keys to segments (the sort .. k_pu_segs of the header), shared with place.hip, which runs it over contigs: E endpoint keys
// group << (pb + 1) | pos << 1 | kind in b.k0 (groups below M < 2^mb, positions 0 .. len[group] < 2^pb) become, per group, the maximal runs
// of equal depth from 0 to len[group] in b.seg_off / seg_start / seg_depth.  ctr[3] = the segments, ctr[4] = the largest depth (an atomicMax:
// zeroed by the caller).  Returns the sorted keys (b.k0 or b.k1).  Everything is queued on the context's stream; nothing synchronises.
// DepthBufs::reserve sizes the set for at most max_keys endpoints of G groups.
void DepthBufs::reserve(int64_t max_keys, int64_t G)
{
    const int64_t ntok_max = max_keys + G;                      // token slots: groups (<= keys) + one per group of the caller
    k0.reserve((size_t)(max_keys + 4) * 8); k1.reserve((size_t)(max_keys + 4) * 8);
    eptr.reserve((size_t)(G + 2) * 4);
    head.reserve((size_t)(max_keys + 2) * 4); hidx.reserve((size_t)(max_keys + 2) * 4); delta.reserve((size_t)(max_keys + 2) * 4); dsum.reserve((size_t)(max_keys + 2) * 4);
    gstart.reserve((size_t)(max_keys + 2) * 4); tok.reserve((size_t)(ntok_max + 2) * 4); tpos.reserve((size_t)(ntok_max + 2) * 4);
    seg_off.reserve((size_t)(G + 2) * 8);
    // segments: at most one per endpoint, plus one per group
    seg_start.reserve((size_t)(ntok_max + 1) * 4); seg_depth.reserve((size_t)(ntok_max + 1) * 4);
}

const uint64_t *depth_segments(Ctx &c, DepthBufs &b, int64_t E, int64_t M, int mb, int pb, const uint32_t *len, unsigned long long *ctr)
{
    hipStream_t s = c.stream;
    uint32_t *eptr = b.eptr.as<uint32_t>(), *head = b.head.as<uint32_t>(), *hidx = b.hidx.as<uint32_t>(), *delta = b.delta.as<uint32_t>();
    uint32_t *dsum = b.dsum.as<uint32_t>(), *gstart = b.gstart.as<uint32_t>(), *tok = b.tok.as<uint32_t>(), *tpos = b.tpos.as<uint32_t>();
    const uint64_t *keys = b.k0.as<uint64_t>();
    if (E > 0) {
        const int which = radix_sort_keys(s, b.k0.as<uint64_t>(), b.k1.as<uint64_t>(), E, 0, mb + pb + 1, c.ws_sort);
        keys = which ? b.k1.as<uint64_t>() : b.k0.as<uint64_t>();
    }
    group_offsets_u32(s, keys, pb + 1, E, eptr, M);             // (E = 0: every pointer 0)
    const int64_t ntok = E + M;                                 // token slots: groups (<= E) + one per read
    ELBA_HIP(hipMemsetAsync(tok, 0, (size_t)(ntok + 1) * 4, s));
    const unsigned nbE = (unsigned)((E + 1 + 255) / 256);
    hipLaunchKernelGGL(k_pu_marks, dim3(nbE), dim3(256), 0, s, keys, eptr, (uint32_t)M, E, head, delta);
    exclusive_scan_u32(s, head, hidx, E + 1, c.ws_scan);
    exclusive_scan_u32(s, delta, dsum, E + 1, c.ws_scan);
    hipLaunchKernelGGL(k_pu_groups, dim3(nbE), dim3(256), 0, s, head, hidx, eptr, (uint32_t)M, E, gstart);
    const int64_t nt = (E > M ? E : M) + 1;
    const unsigned nbt = (unsigned)((nt + 255) / 256);
    hipLaunchKernelGGL(k_pu_tokens, dim3(nbt), dim3(256), 0, s, keys, eptr, hidx, gstart, dsum, len, (uint32_t)M, pb, E, tok);
    exclusive_scan_u32(s, tok, tpos, ntok + 1, c.ws_scan);
    hipLaunchKernelGGL(k_pu_segs, dim3(nbt), dim3(256), 0, s, keys, eptr, hidx, gstart, dsum, len, tok, tpos, (uint32_t)M, pb, ntok,
                       b.seg_off.as<int64_t>(), b.seg_start.as<int32_t>(), b.seg_depth.as<int32_t>(), ctr);
    return keys;
}

void throw_bad_pair(Ctx &c, const GraphInput &in, int64_t a, const char *who)
{
    hipStream_t s = c.stream;
    int64_t r = 0, col = 0; elba_overlap_t o{};
    ELBA_HIP(hipMemcpyAsync(&r, in.rows + a, 8, hipMemcpyDeviceToHost, s));
    ELBA_HIP(hipMemcpyAsync(&col, in.cols + a, 8, hipMemcpyDeviceToHost, s));
    ELBA_HIP(hipMemcpyAsync(&o, in.vals + a, sizeof(o), hipMemcpyDeviceToHost, s));
    ELBA_HIP(hipStreamSynchronize(s));
    throw Error{ELBA_ERR_INVALID_ARG, std::string(who) + ": pair " + std::to_string(a) + " (" + std::to_string(r) + ", " + std::to_string(col) + ") has an interval outside [0, len] or with beg > end: Q [" +
                                          std::to_string(o.begQ) + ", " + std::to_string(o.endQ) + "), T [" + std::to_string(o.begT) + ", " + std::to_string(o.endT) + ")"};
}

void stage_read_pileup(Ctx &c, const elba_pileup_cfg *cfgp)
{
    enter(c.v, EV_READ_PILEUP);
    ELBA_REQUIRE(cfgp, ELBA_ERR_INVALID_ARG, "read_pileup: null cfg");
    const elba_pileup_cfg &cfg = *cfgp;
    ELBA_REQUIRE(cfg.mode == 0 || cfg.mode == 1, ELBA_ERR_INVALID_ARG, "read_pileup: mode must be 0 (passed pairs) or 1 (score > 0)");
    ELBA_REQUIRE(cfg.margin >= 0 && cfg.min_depth >= 1 && cfg.min_run >= 1 && cfg.trim_len >= 0, ELBA_ERR_INVALID_ARG,
                 "read_pileup: need margin >= 0, min_depth >= 1, min_run >= 1, trim_len >= 0");
    const PuInput in = pileup_input(c, "read_pileup");
    const int64_t M = in.M, n = in.n, n4 = 4 * n;
    ELBA_REQUIRE(M < 0x7fffffff && n4 + M < 0xfffffff0ll, ELBA_ERR_UNSUPPORTED, "read_pileup: more than 2^31 reads or 2^30 pairs");
    accepted(c.v, EV_READ_PILEUP);
    hipStream_t s = c.stream;
    int mb = 1, pb = 1;
    while ((1ll << mb) < M + 1) ++mb;
    while ((1ll << pb) < (int64_t)in.maxlen + 1) ++pb;          // positions 0 .. len
    PuParams p{};
    p.rows = in.rows; p.cols = in.cols; p.vals = in.vals; p.n = n; p.len = in.len; p.M = (uint32_t)M; p.pb = pb;
    p.mode = cfg.mode; p.margin = cfg.margin; p.min_depth = cfg.min_depth; p.min_run = cfg.min_run; p.trim_len = cfg.trim_len;
    DepthBufs &db = c.pu.depth;
    db.reserve(n4, M);                                          // keys, marks, scans, tokens and segments for at most 4n endpoints of M reads
    c.pu.ctr.reserve(128);
    c.pu.trim.reserve((size_t)(M + 1) * 8); c.pu.flags.reserve((size_t)M + 4);
    p.keys = db.k0.as<uint64_t>(); p.ctr = c.pu.ctr.as<unsigned long long>();
    c.pu.t_total.start(s);
    ELBA_HIP(hipMemsetAsync(c.pu.ctr.p, 0, 128, s));
    ELBA_HIP(hipMemsetAsync(p.ctr + 2, 0xff, 8, s));
    if (n > 0) hipLaunchKernelGGL(k_pu_emit, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p);
    ELBA_HIP(hipGetLastError());
    unsigned long long h[16] = {0};
    ELBA_HIP(hipMemcpyAsync(h, c.pu.ctr.p, 128, hipMemcpyDeviceToHost, s));
    ELBA_HIP(hipStreamSynchronize(s));
    if (h[2] != ~0ull) throw_bad_pair(c, in, (int64_t)h[2], "read_pileup");
    const int64_t E = 2 * (int64_t)h[1];                        // endpoints
    depth_segments(c, db, E, M, mb, pb, in.len, p.ctr);
    if (M > 0)
        hipLaunchKernelGGL(k_pu_reads, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, db.seg_off.as<int64_t>(), db.seg_start.as<int32_t>(),
                           db.seg_depth.as<int32_t>(), in.len, (uint32_t)M, cfg.min_depth, cfg.min_run, cfg.trim_len, c.pu.trim.as<int2>(), c.pu.flags.as<uint8_t>(), p.ctr);
    ELBA_HIP(hipGetLastError());
    c.pu.t_total.stop(s);
    ELBA_HIP(hipMemcpyAsync(h, c.pu.ctr.p, 128, hipMemcpyDeviceToHost, s));
    ELBA_HIP(hipStreamSynchronize(s));
    elba_pileup_stats st{};
    st.nreads = M; st.pairs = (int64_t)h[0]; st.intervals = (int64_t)h[1]; st.segments = (int64_t)h[3]; st.max_depth = (int64_t)h[4];
    st.unsupported = (int64_t)h[5]; st.split = (int64_t)h[6]; st.trimmed = (int64_t)h[7]; st.trimmed_bases = (int64_t)h[8];
    st.ms_total = c.pu.t_total.ms();
    c.pu.M = M; c.pu.nseg = st.segments; c.pu.n = n; c.pu.stats = st; c.pu.cfg = cfg; done(c.v, EV_READ_PILEUP);
}

void stage_prune_reads(Ctx &c, int mask, int64_t *kept)
{
    enter(c.v, EV_PRUNE_READS);
    ELBA_REQUIRE(mask >= 0 && mask <= 255, ELBA_ERR_INVALID_ARG, "prune_reads: mask must fit in one byte");
    ELBA_REQUIRE(has(c.v, P_PILEUP), ELBA_ERR_STATE, "prune_reads: no pileup of the current overlaps (call elba_read_pileup)");
    const PuInput in = pileup_input(c, "prune_reads");
    ELBA_REQUIRE(in.M == c.pu.M && in.n == c.pu.n, ELBA_ERR_STATE, "prune_reads: the pileup was computed on other overlaps");
    accepted(c.v, EV_PRUNE_READS);
    hipStream_t s = c.stream;
    const int64_t n = in.n;
    c.pu.sel.reserve((size_t)(2 * n + 4) * 4);
    c.pu.rows.reserve((size_t)(n + 1) * 8); c.pu.cols.reserve((size_t)(n + 1) * 8); c.pu.vals.reserve((size_t)(n + 1) * sizeof(elba_overlap_t));
    uint32_t *sel = c.pu.sel.as<uint32_t>(), *pos = sel + (n + 2);
    uint32_t total = 0;
    hipLaunchKernelGGL(k_pu_prune_select, dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), 0, s, in.rows, in.cols, n, c.pu.flags.as<uint8_t>(), (uint8_t)mask, sel);
    exclusive_scan_u32(s, sel, pos, n + 1, c.ws_scan);
    if (n > 0)
        hipLaunchKernelGGL(k_pu_prune_scatter, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, in.rows, in.cols, in.vals, n, sel, pos, c.pu.rows.as<int64_t>(),
                           c.pu.cols.as<int64_t>(), c.pu.vals.as<elba_overlap_t>());
    ELBA_HIP(hipGetLastError());
    ELBA_HIP(hipMemcpyAsync(&total, pos + n, 4, hipMemcpyDeviceToHost, s));
    ELBA_HIP(hipStreamSynchronize(s));
    // the kept pairs become the loaded edge list (elba_set_overlaps' buffers); the context's own alignments stay as they are
    c.tr_in_rows.swap(c.pu.rows); c.tr_in_cols.swap(c.pu.cols); c.tr_in_vals.swap(c.pu.vals);
    c.tr_in_M = in.M; c.tr_in_n = total;
    c.tr_outside = false;                                       // (outside counts belonged to the list the kept pairs replace)
    done(c.v, EV_PRUNE_READS);
    if (kept) *kept = total;
}

}  // namespace elba
