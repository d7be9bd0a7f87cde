// polish.hip — contigs whose bases are voted on by the reads placed on them (elba_polish_contigs; the rule is stated in include/elba_amd.h).
// elba_generate_contigs writes a contig from prefixes of single reads: every error of a chain read stands in it at depth 1.  Here every
// placed read is aligned to its stretch of the contig in a band of W diagonals around its placement (edit distance, free begin and end on
// the contig), the alignments vote per column and per gap, and the columns are called.
//
// Input, all resident: the records of place.hip's place_records (the same launches elba_place_reads runs), the packed reads, of the last
// contig call cg.seq / cg.soff / cg.kind.
//
//   k_po_plan      one lane per read: voter or not, its slice (rows n, first base i0, first column st), the record's first fields; the
//                  rows go through one exclusive scan: the row offset of every voter's choices
//   -- host synchronisation 1: the row offsets (8 bytes per read) and place_records' bad-pair word: the batches are cut on the host --
//   k_po_align<C>  the hot path, W = 64 C: one wavefront per voter, one DP row per step, no LDS.  In band coordinates b = j - i - st + W/2
//                  the diagonal predecessor is the same cell of the row before, the upper one cell b + 1 (one wave_shl:1 between lanes), and
//                  the left dependency inside the row is a scan: H[b] = b + min over e <= b of (cand[e] - e), cand = min(diagonal, up) —
//                  a prefix minimum inside the lane's C cells, six DPP steps over the wavefront (row_shr 1, 2, 4, 8, row_bcast 15, 31), one
//                  wave_shr:1 to make it exclusive.  Cells that do not exist enter as INF and are set to INF again behind the scan.  The
//                  read base of a row is wave-uniform: every 64 rows each lane decodes one base of the packed read (the complement from
//                  the other end on strand 1) and the row takes its base with a readlane.  The contig window slides one base per row: each
//                  lane keeps the codes of its C cells, shifts them by one cell (wave_shl:1 between lanes), and the base that enters at the
//                  top comes from a register filled with 64 consecutive contig bytes every 64 rows — no byte load per lane and row.  The
//                  two bits of a cell's choice are two ballots per cell index; lanes 0 .. 2C-1 store one 64-bit word each: W / 4 bytes per
//                  row, one store instruction.  The end cell: a 64-bit minimum of D << 32 | b.  Lane 0 writes the record and the counts
//   k_po_vote<C>   one wavefront (a workgroup of its own, so that __syncthreads is its only barrier) per voter that was not rejected: blocks
//                  of 64 rows of choices (1 KiB x C, coalesced) and their 64 read bases go to LDS, lane 0 walks back through them and issues
//                  one integer atomic per vote; a run of up steps is held until the step behind it is known, also across blocks
//   k_po_call      one lane per column slot (every contig has L + 1: slot c holds gap c and column c, slot L the gap behind the last
//                  column): the contig by binary search in cg.soff, the five counts of the column and of its left neighbour, 0 .. 2 bases
//   scan           exclusive_scan_u32_to_i64 (prims.hip) over the slots' counts
//   k_po_write     one lane per slot: its bases at its offset; one lane per contig: seq_off
//   -- host synchronisation 2: the output size --
//
// Bounds: a voter has 1 <= n <= len < 2^24 (checked in k_po_plan), its rows lie at toff[r] - toff[ra] + t below the batch's row count, which
// sized the choices (2C words per row); band cells are 0 .. W-1 by construction (lane * C + c); contig bytes are read at pos mod L on a
// circle and only for 0 <= pos < L elsewhere (other cells take code 4, which equals no read base); read bases at i0 + t < i0 + n <= len.
// The walk starts at a cell that exists and follows choices of cells that exist: a diagonal or left step was recorded only with its
// predecessor finite, so 1 <= j <= L there and column j - 1 is below L; gaps are 0 .. L of the contig's L + 1 slots.  The walk still
// checks b in [0, W) and the column before every atomic and raises PQ_ERR instead of writing (ELBA_ERR_INTERNAL): a wrong choice must
// not become a wild store.  Slots are below bases + contigs < 2^32.
// Bytes moved (algorithmic): 24 + 4 bytes per read for the plan, 12 written; per voter 16 bytes of record and slice, n / 4 bytes of packed
// read, n + W contig bytes, n * W / 4 bytes of choices written and read once more by the walk (16 bytes per read base at W = 64), n bytes
// of read codes, one 4-byte atomic per vote (about n + the differences); per slot 40 bytes of counts read, 8 written, 8 through the scan;
// the polished bases once.
#include "common.hpp"
#include <memory>

namespace elba {

namespace {

// counters: 0 voted, 1 rejected, 2 outside, 3 low-depth columns, 4 sum of distances, 5 a walk left its band or contig, 6 a read of 2^24 bases or more
enum { PQ_VOTED = 0, PQ_REJ, PQ_OUT, PQ_LOW, PQ_DIST, PQ_ERR, PQ_LONG, PQ_N = 8 };
constexpr int PO_INF = 1 << 28, PO_BIG = 1 << 27;              // a cell that does not exist or cannot be reached; what no finite distance reaches (n + W < 2^24 + 256)

struct PoPlan { int32_t n, i0, st, pad; };                     // n = 0: no voter

struct PoIn {
    const elba_placement_t *rec; const PoPlan *plan; const int64_t *toff;
    const uint8_t *packed; const uint64_t *byte_off; const uint32_t *len;
    const char *seq; const int64_t *soff; const uint8_t *kind;
    uint32_t ra, rb; int64_t tbase;                            // the batch's reads [ra, rb) and toff[ra]
    int max_diff_q16;
};

__device__ __forceinline__ int po_read_base(const uint8_t *mem, uint32_t i) { return (mem[i >> 2] >> (6 - 2 * (i & 3))) & 3; }    // the layout of align.hip's base_at
// the code of contig position pos (0 A, 1 C, 2 G, 3 T from the ASCII bytes of cg.seq), 4 where a path contig has no such column
__device__ __forceinline__ int po_contig_code(const char *s, int pos, int L, bool circ)
{
    if (circ) { pos %= L; if (pos < 0) pos += L; }
    else if (pos < 0 || pos >= L) return 4;
    const int x = ((unsigned char)s[pos] >> 1) & 3;            // A 0, C 1, T 2, G 3
    return x ^ (x >> 1);
}
__device__ __forceinline__ int po_mod(int x, int L) { x %= L; return x < 0 ? x + L : x; }

__device__ __forceinline__ int po_shl1(int v, int fill) { return __builtin_amdgcn_update_dpp(fill, v, 0x130 /* wave_shl:1 */, 0xf, 0xf, false); }     // lane l takes lane l + 1
__device__ __forceinline__ int po_shr1(int v, int fill) { return __builtin_amdgcn_update_dpp(fill, v, 0x138 /* wave_shr:1 */, 0xf, 0xf, false); }     // lane l takes lane l - 1
// inclusive prefix minimum over the wavefront in registers: four steps inside every row of 16 lanes, two row broadcasts
__device__ __forceinline__ int po_wave_min_scan(int v)
{
    int t;
    t = __builtin_amdgcn_update_dpp(PO_INF, v, 0x111 /* row_shr:1 */, 0xf, 0xf, false); v = t < v ? t : v;
    t = __builtin_amdgcn_update_dpp(PO_INF, v, 0x112 /* row_shr:2 */, 0xf, 0xf, false); v = t < v ? t : v;
    t = __builtin_amdgcn_update_dpp(PO_INF, v, 0x114 /* row_shr:4 */, 0xf, 0xf, false); v = t < v ? t : v;
    t = __builtin_amdgcn_update_dpp(PO_INF, v, 0x118 /* row_shr:8 */, 0xf, 0xf, false); v = t < v ? t : v;
    t = __builtin_amdgcn_update_dpp(PO_INF, v, 0x142 /* row_bcast:15 */, 0xa, 0xf, false); v = t < v ? t : v;
    t = __builtin_amdgcn_update_dpp(PO_INF, v, 0x143 /* row_bcast:31 */, 0xc, 0xf, false); v = t < v ? t : v;
    return v;
}

__device__ __forceinline__ unsigned long long po_wave_count(bool b) { return (unsigned long long)__builtin_popcountll(__ballot(b)); }

__global__ void k_po_plan(const elba_placement_t *rec, const uint32_t *len, const uint32_t *clen, const uint8_t *kind, uint32_t M, PoPlan *plan, uint32_t *rows,
                          elba_polish_read_t *out, unsigned long long *ctr)
{
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    bool outside = false, toolong = false;
    if (r < M) {
        const elba_placement_t p = rec[r];
        PoPlan pl{0, 0, 0, 0};
        elba_polish_read_t o{0, 0, 0, ELBA_POLISH_NOT_PLACED};
        if (p.kind) {
            if (p.flags & 2) { outside = true; o.status = ELBA_POLISH_OUTSIDE; }
            else {
                const int64_t l = len[r], L = clen[p.contig];
                int64_t i0 = 0, i1;
                if (kind[p.contig] == 1) i1 = l < L ? l : L;
                else { i0 = p.start < 0 ? -p.start : 0; i1 = L - p.start < l ? L - p.start : l; }
                if (l >= (1 << 24)) toolong = true;
                else { pl.n = (int32_t)(i1 - i0); pl.i0 = (int32_t)i0; pl.st = (int32_t)(p.start + i0); o.n = pl.n; }
            }
        }
        plan[r] = pl; rows[r] = (uint32_t)pl.n; out[r] = o;
    }
    const unsigned long long no = po_wave_count(outside), nl = po_wave_count(toolong);
    if ((threadIdx.x & 63) == 0) {
        if (no) atomicAdd(&ctr[PQ_OUT], no);
        if (nl) atomicAdd(&ctr[PQ_LONG], nl);
    }
}

constexpr int PO_ALIGN_WAVES = 4;       // independent wavefronts per workgroup

template <int C>
__global__ __launch_bounds__(64 * PO_ALIGN_WAVES) void k_po_align(PoIn g, unsigned long long *trace, elba_polish_read_t *out, unsigned long long *cstat, unsigned long long *ctr)
{
    constexpr int W = 64 * C;
    const int lane = threadIdx.x & 63;
    const uint32_t r = (uint32_t)__builtin_amdgcn_readfirstlane((int)(g.ra + blockIdx.x * PO_ALIGN_WAVES + (threadIdx.x >> 6)));
    if (r >= g.rb) return;
    const PoPlan pl = g.plan[r];
    if (pl.n == 0) return;                                      // (wave-uniform: every lane below is active, which the DPP steps need)
    const elba_placement_t p = g.rec[r];
    const int n = pl.n, L = (int)(g.soff[p.contig + 1] - g.soff[p.contig]);
    const bool circ = g.kind[p.contig] == 1, rcs = p.strand != 0;
    const char *s = g.seq + g.soff[p.contig];
    const uint8_t *src = g.packed + g.byte_off[r];
    const uint32_t l = g.len[r];
    unsigned long long *tr = trace + (size_t)(g.toff[r] - g.tbase) * (2 * C);
    const int base0 = pl.st - W / 2;                            // column j of cell b in row i: base0 + i + b
    const int b0 = lane * C;
    int P[C], cb[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int j = base0 + b0 + c;                           // row 0
        P[c] = (circ || (j >= 0 && j <= L)) ? 0 : PO_INF;
        cb[c] = po_contig_code(s, j, L, circ);                  // row 1 compares with s[j - 1], j = base0 + 1 + b
    }
    int rbv = 0, nxt = 0;
    for (int t = 0; t < n; ++t) {                               // row i = t + 1
        if ((t & 63) == 0) {
            const int x = t + lane;
            if (x < n) { const uint32_t idx = (uint32_t)(pl.i0 + x); rbv = rcs ? 3 - po_read_base(src, l - 1 - idx) : po_read_base(src, idx); }
        }
        if (t >= 1) {                                           // the window slides: cell b takes what cell b + 1 compared with, the top cell the base that enters
            if (((t - 1) & 63) == 0) nxt = po_contig_code(s, base0 + t + W - 1 + lane, L, circ);
            const int in = __builtin_amdgcn_readlane(nxt, (t - 1) & 63);
            const int fromup = po_shl1(cb[0], in);
#pragma unroll
            for (int c = 0; c + 1 < C; ++c) cb[c] = cb[c + 1];
            cb[C - 1] = fromup;
        }
        const int qb = __builtin_amdgcn_readlane(rbv, t & 63);
        const int up0 = po_shl1(P[0], PO_INF);
        int dg[C], up[C], m[C], run = PO_INF;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            dg[c] = P[c] + (cb[c] != qb ? 1 : 0);
            up[c] = (c + 1 < C ? P[c + 1] : up0) + 1;
            const int cand = dg[c] < up[c] ? dg[c] : up[c];
            const int v = cand - (b0 + c);
            run = v < run ? v : run;
            m[c] = run;                                         // the prefix minimum inside the lane
        }
        const int excl = po_shr1(po_wave_min_scan(m[C - 1]), PO_INF);
        unsigned long long lo[C], hi[C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const int j = base0 + t + 1 + b0 + c;
            int h = (b0 + c) + (m[c] < excl ? m[c] : excl);
            if (!(circ || (j >= 0 && j <= L)) || h > PO_BIG) h = PO_INF;
            const int ch = dg[c] == h ? 0 : (up[c] == h ? 1 : 2);
            lo[c] = __ballot(ch & 1); hi[c] = __ballot(ch >> 1);
            P[c] = h;
        }
        unsigned long long wv = 0;
#pragma unroll
        for (int c = 0; c < C; ++c) { if (lane == 2 * c) wv = lo[c]; if (lane == 2 * c + 1) wv = hi[c]; }
        if (lane < 2 * C) tr[(size_t)t * (2 * C) + lane] = wv;
    }
    // the end cell: the smallest D of row n, of equal ones the smallest band cell
    unsigned long long key = ~0ull;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const unsigned long long k = ((unsigned long long)(unsigned)P[c] << 32) | (unsigned)(b0 + c);
        if (P[c] < PO_INF && k < key) key = k;
    }
    for (int o = 32; o >= 1; o >>= 1) { const unsigned long long k = (unsigned long long)__shfl_xor((long long)key, o); if (k < key) key = k; }
    if (lane == 0) {
        const int dist = (int)(key >> 32), bend = (int)(uint32_t)key;
        const bool rej = (long long)dist > (((long long)g.max_diff_q16 * n) >> 16);
        out[r] = elba_polish_read_t{dist, n, base0 + n + bend, rej ? ELBA_POLISH_REJECTED : ELBA_POLISH_VOTED};
        atomicAdd(&ctr[rej ? PQ_REJ : PQ_VOTED], 1ull);
        if (!rej) { if (dist) atomicAdd(&ctr[PQ_DIST], (unsigned long long)dist); atomicAdd(&cstat[4 * (size_t)p.contig], 1ull); }
    }
}

constexpr int PO_VOTE_ROWS = 64;        // rows of choices per LDS block

template <int C>
__global__ __launch_bounds__(64) void k_po_vote(PoIn g, const unsigned long long *trace, const elba_polish_read_t *out, uint32_t *col, uint32_t *gap, unsigned long long *ctr)
{
    constexpr int W = 64 * C;
    __shared__ unsigned long long rows[PO_VOTE_ROWS * 2 * C];
    __shared__ uint8_t qrow[PO_VOTE_ROWS];
    const int lane = threadIdx.x;
    const uint32_t r = g.ra + blockIdx.x;
    if (r >= g.rb) return;
    const PoPlan pl = g.plan[r];
    if (pl.n == 0) return;
    const elba_polish_read_t rr = out[r];
    if (rr.status != ELBA_POLISH_VOTED) return;                 // (all three exits are the same for the whole workgroup)
    const elba_placement_t p = g.rec[r];
    const int n = pl.n, L = (int)(g.soff[p.contig + 1] - g.soff[p.contig]);
    const bool circ = g.kind[p.contig] == 1, rcs = p.strand != 0;
    const uint8_t *src = g.packed + g.byte_off[r];
    const uint32_t l = g.len[r];
    const unsigned long long *tr = trace + (size_t)(g.toff[r] - g.tbase) * (2 * C);
    uint32_t *mycol = col + 5 * (size_t)g.soff[p.contig], *mygap = gap + 4 * (size_t)(g.soff[p.contig] + p.contig);
    const int base0 = pl.st - W / 2;
    int i = n, j = rr.end_j, pend = -1;                         // lane 0's walk; pend: the base of the last up step of a run that has not ended yet
    bool bad = false;
    for (int hiRow = n; hiRow >= 1; hiRow -= PO_VOTE_ROWS) {    // rows loRow .. hiRow; row i is entry t = i - 1 of the read's choices
        const int loRow = hiRow - PO_VOTE_ROWS + 1 > 1 ? hiRow - PO_VOTE_ROWS + 1 : 1;
        const int nw = (hiRow - loRow + 1) * 2 * C;
        for (int x = lane; x < nw; x += 64) rows[x] = tr[(size_t)(loRow - 1) * (2 * C) + x];
        if (loRow + lane <= hiRow) { const uint32_t idx = (uint32_t)(pl.i0 + loRow + lane - 1); qrow[lane] = (uint8_t)(rcs ? 3 - po_read_base(src, l - 1 - idx) : po_read_base(src, idx)); }
        __syncthreads();
        if (lane == 0 && !bad) {
            while (i >= loRow) {
                const int b = j - i - base0;
                if (b < 0 || b >= W) { bad = true; break; }
                const int c = b % C, d = b / C, row = i - loRow;
                const int ch = (int)((rows[row * 2 * C + 2 * c] >> d) & 1) | ((int)((rows[row * 2 * C + 2 * c + 1] >> d) & 1) << 1);
                const int qb = qrow[row];
                if (ch == 1) { pend = qb; --i; continue; }
                if (pend >= 0) { const int gp = circ ? po_mod(j, L) : j; if (gp < 0 || gp > L) { bad = true; break; } atomicAdd(&mygap[4 * (size_t)gp + pend], 1u); pend = -1; }
                const int cp = circ ? po_mod(j - 1, L) : j - 1;
                if (cp < 0 || cp >= L) { bad = true; break; }
                if (ch == 0) { atomicAdd(&mycol[5 * (size_t)cp + qb], 1u); --i; --j; }
                else { atomicAdd(&mycol[5 * (size_t)cp + 4], 1u); --j; }
            }
        }
        __syncthreads();
    }
    if (lane == 0) {
        if (!bad && pend >= 0) { const int gp = circ ? po_mod(j, L) : j; if (gp < 0 || gp > L) bad = true; else atomicAdd(&mygap[4 * (size_t)gp + pend], 1u); }
        if (bad) atomicAdd(&ctr[PQ_ERR], 1ull);
    }
}

__device__ __forceinline__ uint32_t po_depth(const uint32_t *c5) { return c5[0] + c5[1] + c5[2] + c5[3] + c5[4]; }

// slot x of the bases + nc slots: contig k = the last with soff[k] + k <= x, slot = x - soff[k] - k in 0 .. L
__global__ void k_po_call(const char *seq, const int64_t *soff, const uint8_t *kind, int64_t nc, int64_t X, const uint32_t *col, const uint32_t *gap, int min_depth,
                          uint32_t *cnt, uint32_t *emit, unsigned long long *cstat, unsigned long long *ctr)
{
    const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool low = false;
    if (x < X) {
        int64_t lo = 0, hi = nc - 1;
        while (lo < hi) { const int64_t mid = (lo + hi + 1) >> 1; if (soff[mid] + mid <= x) lo = mid; else hi = mid - 1; }
        const int64_t k = lo, L = soff[k + 1] - soff[k], slot = x - soff[k] - k;
        const bool circ = kind[k] == 1;
        const uint32_t *c5 = col + 5 * soff[k], *g4 = gap + 4 * (soff[k] + k + slot);
        uint32_t n = 0, word = 0;
        // the gap in front of this slot
        if (L > 0 && (slot < L || !circ)) {
            uint32_t span;
            if (slot == L) span = po_depth(c5 + 5 * (L - 1));
            else {
                span = po_depth(c5 + 5 * slot);
                if (slot > 0 || circ) { const uint32_t left = po_depth(c5 + 5 * (slot > 0 ? slot - 1 : L - 1)); if (left < span) span = left; }
            }
            const uint32_t sum = g4[0] + g4[1] + g4[2] + g4[3];
            if (2ull * sum > span) {
                int best = 0;
                for (int b = 1; b < 4; ++b) if (g4[b] > g4[best]) best = b;
                word |= (uint32_t)(uint8_t)"ACGT"[best] << (8 * n++);
                atomicAdd(&cstat[4 * k + 3], 1ull);
            }
        }
        if (slot < L) {
            const uint32_t *cc = c5 + 5 * slot;
            const int own = po_contig_code(seq + soff[k], (int)slot, (int)L, false);
            if (po_depth(cc) < (uint32_t)min_depth) { low = true; word |= (uint32_t)(uint8_t)seq[soff[k] + slot] << (8 * n++); }
            else {
                int best = own;                                   // the contig's own base, then A, C, G, T, then the deletion
                for (int b = 0; b < 5; ++b) if (cc[b] > cc[best]) best = b;
                if (best == 4) atomicAdd(&cstat[4 * k + 2], 1ull);
                else { word |= (uint32_t)(uint8_t)"ACGT"[best] << (8 * n++); if (best != own) atomicAdd(&cstat[4 * k + 1], 1ull); }
            }
        }
        cnt[x] = n; emit[x] = word;
    }
    const unsigned long long nl = po_wave_count(low);
    if ((threadIdx.x & 63) == 0 && nl) atomicAdd(&ctr[PQ_LOW], nl);
}

__global__ void k_po_write(const uint32_t *cnt, const uint32_t *emit, const int64_t *off, const int64_t *soff, int64_t nc, int64_t X, char *out, int64_t *seq_off)
{
    const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x <= nc) seq_off[x] = off[soff[x] + x];
    if (x >= X) return;
    const uint32_t n = cnt[x], w = emit[x];
    const int64_t o = off[x];
    if (n >= 1) out[o] = (char)(w & 0xff);
    if (n >= 2) out[o + 1] = (char)((w >> 8) & 0xff);
}

template <int C>
void po_launch_batch(hipStream_t s, const PoIn &g, unsigned long long *trace, elba_polish_read_t *rec, uint32_t *col, uint32_t *gap, unsigned long long *cstat, unsigned long long *ctr,
                     hipEvent_t e0, hipEvent_t e1)
{
    const uint32_t nr = g.rb - g.ra;
    ELBA_HIP(hipEventRecord(e0, s));
    hipLaunchKernelGGL(k_po_align<C>, dim3((nr + PO_ALIGN_WAVES - 1) / PO_ALIGN_WAVES), dim3(64 * PO_ALIGN_WAVES), 0, s, g, trace, rec, cstat, ctr);
    ELBA_HIP(hipEventRecord(e1, s));
    hipLaunchKernelGGL(k_po_vote<C>, dim3(nr), dim3(64), 0, s, g, (const unsigned long long *)trace, (const elba_polish_read_t *)rec, col, gap, ctr);
}

struct PoEvents {
    std::vector<hipEvent_t> e;
    void grow(size_t n) { while (e.size() < n) { hipEvent_t x; ELBA_HIP(hipEventCreate(&x)); e.push_back(x); } }
    ~PoEvents() { for (hipEvent_t x : e) (void)hipEventDestroy(x); }
};

}  // namespace

void stage_polish_contigs(Ctx &c, const elba_polish_cfg *cfg, elba_polished_t *out)
{
    c.po.for_cg = 0;                                               // (whatever this call ends in, the counts of the one before are gone)
    ELBA_REQUIRE(cfg, ELBA_ERR_INVALID_ARG, "polish_contigs: null cfg");
    ELBA_REQUIRE(!cfg->reserved[0] && !cfg->reserved[1] && !cfg->reserved[2], ELBA_ERR_INVALID_ARG, "polish_contigs: reserved words must be 0");
    ELBA_REQUIRE(cfg->skip_flags >= 0 && cfg->skip_flags <= 255, ELBA_ERR_INVALID_ARG, "polish_contigs: skip_flags must fit in one byte");
    ELBA_REQUIRE(cfg->band == 64 || cfg->band == 128 || cfg->band == 256, ELBA_ERR_INVALID_ARG, "polish_contigs: band is 64, 128 or 256");
    ELBA_REQUIRE(cfg->max_diff_q16 >= 0 && cfg->max_diff_q16 <= 65536, ELBA_ERR_INVALID_ARG, "polish_contigs: max_diff_q16 is 0 .. 65536");
    ELBA_REQUIRE(cfg->min_depth >= 1, ELBA_ERR_INVALID_ARG, "polish_contigs: min_depth is at least 1");
    ELBA_REQUIRE((cfg->flags & ~ELBA_POLISH_EXPORT_VOTES) == 0, ELBA_ERR_INVALID_ARG, "polish_contigs: unknown flags");
    const PlaceWork w = place_records(c, cfg->skip_flags, "polish_contigs", false, &c.po.t_total);
    const int64_t M = w.M, nc = w.nc, bases = c.cg.bases, X = bases + nc;
    const int W = cfg->band;
    ELBA_REQUIRE(c.cg.stats.longest < (1ll << 30), ELBA_ERR_UNSUPPORTED, "polish_contigs: a contig of 2^30 bases or more");
    ELBA_REQUIRE(5 * bases + 4 * nc < 0xfffffff0ll, ELBA_ERR_UNSUPPORTED, "polish_contigs: 5 x contig bases + 4 x contigs reach 2^32");
    hipStream_t s = c.stream;
    c.po.plan.reserve((size_t)(M + 1) * sizeof(PoPlan)); c.po.rec.reserve((size_t)(M + 1) * sizeof(elba_polish_read_t)); c.po.cnt.reserve((size_t)((M > X ? M : X) + 2) * 4);
    c.po.toff.reserve((size_t)(M + 2) * 8); c.po.col.reserve((size_t)(5 * bases + 8) * 4); c.po.gap.reserve((size_t)(4 * X + 8) * 4); c.po.emit.reserve((size_t)(X + 2) * 4);
    c.po.off.reserve((size_t)(X + 2) * 8); c.po.cstat.reserve((size_t)(4 * nc + 4) * 8); c.po.seqoff.reserve((size_t)(nc + 2) * 8); c.po.ctr.reserve(PQ_N * 8);
    PoPlan *plan = c.po.plan.as<PoPlan>();
    elba_polish_read_t *rec = c.po.rec.as<elba_polish_read_t>();
    uint32_t *cnt = c.po.cnt.as<uint32_t>(), *col = c.po.col.as<uint32_t>(), *gap = c.po.gap.as<uint32_t>(), *emit = c.po.emit.as<uint32_t>();
    int64_t *toff = c.po.toff.as<int64_t>(), *off = c.po.off.as<int64_t>(), *seqoff = c.po.seqoff.as<int64_t>();
    unsigned long long *cstat = c.po.cstat.as<unsigned long long>(), *ctr = c.po.ctr.as<unsigned long long>();
    ELBA_HIP(hipMemsetAsync(ctr, 0, PQ_N * 8, s));
    ELBA_HIP(hipMemsetAsync(cstat, 0, (size_t)(4 * nc + 4) * 8, s));
    ELBA_HIP(hipMemsetAsync(col, 0, (size_t)(5 * bases + 8) * 4, s));
    ELBA_HIP(hipMemsetAsync(gap, 0, (size_t)(4 * X + 8) * 4, s));
    ELBA_HIP(hipMemsetAsync(cnt, 0, (size_t)(M + 2) * 4, s));
    if (M > 0)
        hipLaunchKernelGGL(k_po_plan, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, (const elba_placement_t *)w.rec, w.src.len, w.clen, c.cg.kind.as<uint8_t>(), (uint32_t)M, plan, cnt, rec, ctr);
    exclusive_scan_u32_to_i64(s, cnt, toff, M + 1, c.ws_scan);
    ELBA_HIP(hipGetLastError());
    // synchronisation 1: the row offsets of the voters' choices, place_records' bad-pair word, the reads that are too long
    std::vector<int64_t> h_toff((size_t)M + 1);
    unsigned long long hp[PLACE_CTR_WORDS] = {0}, hq[PQ_N] = {0};
    ELBA_HIP(hipMemcpyAsync(h_toff.data(), toff, (size_t)(M + 1) * 8, hipMemcpyDeviceToHost, s));
    ELBA_HIP(hipMemcpyAsync(hp, w.ctr, PLACE_CTR_WORDS * 8, hipMemcpyDeviceToHost, s));
    ELBA_HIP(hipMemcpyAsync(hq, ctr, PQ_N * 8, hipMemcpyDeviceToHost, s));
    ELBA_HIP(hipStreamSynchronize(s));
    if (hp[PLACE_CTR_BAD] != ~0ull) throw_bad_pair(c, w.in, (int64_t)hp[PLACE_CTR_BAD], "polish_contigs");
    ELBA_REQUIRE(hq[PQ_LONG] == 0, ELBA_ERR_UNSUPPORTED, "polish_contigs: a placed read of 2^24 bases or more");
    // the batches: consecutive reads whose choices fit the cap; a read that alone exceeds it is a batch of its own
    int64_t cap = c.opt.polish_trace_bytes;
    if (cap <= 0) {
        size_t free_b = 0, total_b = 0;
        ELBA_HIP(hipMemGetInfo(&free_b, &total_b));
        cap = (int64_t)((free_b + c.po.trace.cap) / 8);
        if (cap < (64ll << 20)) cap = 64ll << 20;
    }
    const int64_t row_bytes = W / 4, cap_rows = cap / row_bytes;
    std::vector<std::pair<uint32_t, uint32_t>> batches;
    int64_t most = 0;
    for (int64_t ra = 0; ra < M;) {
        int64_t rb = ra;
        while (rb < M && h_toff[(size_t)rb + 1] - h_toff[(size_t)ra] <= cap_rows) ++rb;
        if (rb == ra) rb = ra + 1;
        const int64_t rows = h_toff[(size_t)rb] - h_toff[(size_t)ra];
        if (rows > 0) { batches.emplace_back((uint32_t)ra, (uint32_t)rb); if (rows > most) most = rows; }
        ra = rb;
    }
    c.po.trace.reserve((size_t)most * row_bytes + 64);
    PoEvents ev;
    ev.grow(2 * batches.size());
    PoIn g{w.rec, plan, toff, w.src.packed, w.src.byte_off, w.src.len, c.cg.seq.as<char>(), c.cg.soff.as<int64_t>(), c.cg.kind.as<uint8_t>(), 0, 0, 0, cfg->max_diff_q16};
    unsigned long long *trace = c.po.trace.as<unsigned long long>();
    for (size_t b = 0; b < batches.size(); ++b) {
        g.ra = batches[b].first; g.rb = batches[b].second; g.tbase = h_toff[g.ra];
        if (W == 64) po_launch_batch<1>(s, g, trace, rec, col, gap, cstat, ctr, ev.e[2 * b], ev.e[2 * b + 1]);
        else if (W == 128) po_launch_batch<2>(s, g, trace, rec, col, gap, cstat, ctr, ev.e[2 * b], ev.e[2 * b + 1]);
        else po_launch_batch<4>(s, g, trace, rec, col, gap, cstat, ctr, ev.e[2 * b], ev.e[2 * b + 1]);
    }
    ELBA_HIP(hipMemsetAsync(cnt, 0, (size_t)(X + 2) * 4, s));
    if (X > 0 && nc > 0)
        hipLaunchKernelGGL(k_po_call, dim3((unsigned)((X + 255) / 256)), dim3(256), 0, s, c.cg.seq.as<char>(), c.cg.soff.as<int64_t>(), c.cg.kind.as<uint8_t>(), nc, X, (const uint32_t *)col,
                           (const uint32_t *)gap, cfg->min_depth, cnt, emit, cstat, ctr);
    exclusive_scan_u32_to_i64(s, cnt, off, X + 1, c.ws_scan);
    c.po.seq.reserve((size_t)(2 * X + 64));                     // (a slot emits two bases at most)
    if (nc > 0)
        hipLaunchKernelGGL(k_po_write, dim3((unsigned)((X + 1 + 255) / 256)), dim3(256), 0, s, (const uint32_t *)cnt, (const uint32_t *)emit, (const int64_t *)off, c.cg.soff.as<int64_t>(), nc, X,
                           c.po.seq.as<char>(), seqoff);
    else ELBA_HIP(hipMemsetAsync(seqoff, 0, 8, s));             // (no contig: cg.soff may not be there)
    ELBA_HIP(hipGetLastError());
    c.po.t_total.stop(s);
    // synchronisation 2: the output size (with the offsets and the counts)
    const bool votes = (cfg->flags & ELBA_POLISH_EXPORT_VOTES) != 0;
    elba_polished_t &o = *out;                                  // (zeroed by the caller; every block lands in it at once, so that elba_free_polished releases what a failed allocation or copy leaves)
    o.n = nc; o.nreads = votes ? M : 0;
    o.seq_off = host_block<int64_t>((size_t)nc + 1);
    std::vector<unsigned long long> h_cstat((size_t)(4 * nc + 4));
    copy_out(c, o.seq_off, seqoff, (size_t)nc + 1);
    ELBA_HIP(hipMemcpyAsync(h_cstat.data(), cstat, (size_t)(4 * nc + 4) * 8, hipMemcpyDeviceToHost, s));
    ELBA_HIP(hipMemcpyAsync(hq, ctr, PQ_N * 8, hipMemcpyDeviceToHost, s));
    ELBA_HIP(hipStreamSynchronize(s));
    ELBA_REQUIRE(hq[PQ_ERR] == 0, ELBA_ERR_INTERNAL, "polish_contigs: a walk through the choices left its band or its contig");
    const int64_t after = o.seq_off[nc];
    ELBA_REQUIRE(after >= 0 && after <= 2 * X, ELBA_ERR_INTERNAL, "polish_contigs: the offsets do not end inside the polished bases");
    o.seq = host_block<char>((size_t)after);
    o.voters = host_block<int64_t>((size_t)nc); o.substituted = host_block<int64_t>((size_t)nc); o.deleted = host_block<int64_t>((size_t)nc); o.inserted = host_block<int64_t>((size_t)nc);
    for (int64_t k = 0; k < nc; ++k) {
        o.voters[k] = (int64_t)h_cstat[(size_t)(4 * k)]; o.substituted[k] = (int64_t)h_cstat[(size_t)(4 * k + 1)];
        o.deleted[k] = (int64_t)h_cstat[(size_t)(4 * k + 2)]; o.inserted[k] = (int64_t)h_cstat[(size_t)(4 * k + 3)];
    }
    copy_out(c, o.seq, c.po.seq.p, (size_t)after);
    if (votes) {
        o.col_off = host_block<int64_t>((size_t)nc + 1); o.col = host_block<uint32_t>((size_t)(5 * bases)); o.gap = host_block<uint32_t>((size_t)(4 * X)); o.reads = host_block<elba_polish_read_t>((size_t)M);
        copy_out(c, o.col_off, c.cg.soff.p, (size_t)nc + 1);
        copy_out(c, o.col, col, (size_t)(5 * bases)); copy_out(c, o.gap, gap, (size_t)(4 * X)); copy_out(c, o.reads, rec, (size_t)M);
    }
    ELBA_HIP(hipStreamSynchronize(s));
    elba_polish_stats st{};
    st.nreads = M; st.voted = (int64_t)hq[PQ_VOTED]; st.rejected = (int64_t)hq[PQ_REJ]; st.outside = (int64_t)hq[PQ_OUT]; st.low_depth_columns = (int64_t)hq[PQ_LOW];
    st.bases_before = bases; st.bases_after = after; st.sum_dist = (int64_t)hq[PQ_DIST]; st.cells = h_toff[(size_t)M] * W; st.batches = (int64_t)batches.size();
    st.ms_total = c.po.t_total.ms();
    for (size_t b = 0; b < batches.size(); ++b) { float t = 0; ELBA_HIP(hipEventElapsedTime(&t, ev.e[2 * b], ev.e[2 * b + 1])); st.ms_align += t; }
    c.po.stats = st; c.po.for_cg = c.cg.serial;
}

}  // namespace elba
