// induce.hip — the induced sub-problem of one part (elba_induce_part): what the reference's GetInducedReadSequences and
// ImposeMyReadDistribution (src/ContigGeneration.cpp) do with local_proc_assignments — the reads of part p and the pairs between them,
// renumbered densely — cut out on the device, with the counts of the pairs that leave the part, so that the part's bad-read rule is the
// whole run's (elba_set_outside_counts, tr.hip).  The rule is stated in include/elba_amd.h.  An export: it reads the graph's input as
// graph_input() names it and the bases through read_source(), changes no product and invalidates nothing.
//
//   k_in_select         one lane per read v <= M: sel[v] = (part_of_read[v] == part), bytes[v] = the packed bytes of a selected read
//                       ((len + 3) / 4; 0 without ELBA_INDUCE_BASES); the selected bases, one atomic per wavefront
//   scans               sel -> first (u32): the NEW id of a selected read — new_of_old is this array, no second copy —, first[M] = reads;
//                       bytes -> boff (i64): the first output byte of every read, boff[M] = packed_bytes
//   k_in_pairs_mark     one lane per pair a <= n: keep[a] = both reads selected.  A pair with exactly one read selected adds 1 to that
//                       read's outside_aligned (and to outside_passed when passed != 0): atomicAdd on the counters of the NEW id.  Such
//                       pairs are few by construction (a partition by components of the passed pairs splits failed pairs only).  The two
//                       totals take one atomic per wavefront and counter, through ballots as in tr.hip
//   scan                keep -> pos (u32), pos[n] = pairs
//   -- host synchronisation 1: reads, pairs, packed_bytes (they size the results) --
//   k_in_reads          one lane per read: old_of_new[first[v]] = v, and with the bases len', byte_off' and srcb = 4 x the read's source
//                       byte offset (the first base of the read counted from the start of the source buffer)
//   k_in_pairs_scatter  one lane per pair: a kept pair goes to pos[a] — 16 bytes of new ids and the 36-byte record as nine dwords (the
//                       records are 4-byte aligned, not 16: no wider access is legal), so the output keeps the input's order
//   k_trim_repack       (repack.hpp, the kernel of trim.hip, with every piece a whole read: beg = 0) the 2-bit gather, flat over the output
//   -- host synchronisation 2: the counters (bases, split_pairs, split_passed); a third one behind the host copies of ELBA_INDUCE_HOST --
//
// Every value is an integer and every atomic an integer add: the result does not depend on the order in which they arrive.
// Bounds.  Reads v < M tested before part / len / src_off; sel, bytes, first have M + 1 entries (entry M: 0, the scans' totals), boff M + 1.
// Pairs a < n tested before rows / cols / vals; keep and pos have n + 1 entries.  An end of a pair that is not below M counts as not
// selected (a loaded list was checked when it was loaded, own alignments are below M by construction: the test costs nothing).  The new id
// first[v] of a selected read is below reads <= M: old_of_new, len', byte_off', srcb have reads + 1 entries, the outside counters M + 1
// (zeroed before the mark, which runs before reads is known).  pos[a] of a kept pair is below pairs: rows', cols', vals' have pairs + 1.
// The gather's bounds are trim.hip's: the output holds packed_bytes + 16 bytes, the bytes from packed_bytes & ~7 on are zeroed before the
// kernel; a read of length 0 has no byte (repack.hpp says why it is harmless) and its source offset is at most the source's packed bytes:
// the two aligned words read there end inside the source's 16 guard bytes.  No grid is capped: every kernel has one lane per read, per
// pair or per output word.
// Bytes moved (algorithmic): 4 B of part_of_read per read (host to device, then read once) + 4 B of its length, 4 + 4 B written and the two
// scans (8 and 12 B per read); 16 B per pair read by the mark + 1 B (`passed`) of a pair with one read selected, 4 B written, the scan
// (8 B per pair); per selected read 28 B written by k_in_reads (8 old_of_new, 4 len', 8 byte_off', 8 srcb) from 16 B read; 52 B read and
// 52 B written per kept pair (+ 8 B of keep / pos per input pair); bases / 4 read and bases / 4 written by the gather, + 16 B per read
// (byte_off' + srcb; len' where a read ends).
#include "common.hpp"
#include "repack.hpp"

namespace elba {

namespace {

constexpr int IN_THREADS = 256;
using u64 = unsigned long long;
enum { IN_BASES = 0, IN_SPLIT = 1, IN_SPLIT_PASSED = 2, IN_CTR = 8 };      // ctr[]

__global__ __launch_bounds__(IN_THREADS) void k_in_select(const int32_t *part, int32_t want, const uint32_t *len, int64_t M, uint32_t *sel, uint32_t *bytes, u64 *ctr)
{
    const int64_t v = (int64_t)blockIdx.x * IN_THREADS + threadIdx.x;
    u64 bases = 0;
    if (v <= M) {
        const bool on = v < M && part[v] == want;
        const uint32_t l = on && len ? len[v] : 0u;
        sel[v] = on ? 1u : 0u; bytes[v] = (l + 3u) >> 2;
        bases = l;
    }
    for (int o = 32; o >= 1; o >>= 1) bases += (u64)__shfl_xor((long long)bases, o);
    if ((threadIdx.x & 63) == 0 && bases) atomicAdd(&ctr[IN_BASES], bases);
}

__global__ __launch_bounds__(IN_THREADS) void k_in_pairs_mark(const int64_t *rows, const int64_t *cols, const elba_overlap_t *vals, int64_t n, int64_t M, const uint32_t *sel,
                                                              const uint32_t *first, uint32_t *keep, uint32_t *oa, uint32_t *op, u64 *ctr)
{
    const int64_t a = (int64_t)blockIdx.x * IN_THREADS + threadIdx.x;
    bool split = false, split_passed = false;
    if (a < n) {
        const int64_t r = rows[a], c = cols[a];
        const bool sr = r >= 0 && r < M && sel[r], sc = c >= 0 && c < M && sel[c];
        keep[a] = sr && sc ? 1u : 0u;
        if (sr != sc) {
            const uint32_t w = first[sr ? r : c];                  // the new id of the selected end (< reads <= M)
            split = true; split_passed = vals[a].passed != 0;
            atomicAdd(&oa[w], 1u);
            if (split_passed) atomicAdd(&op[w], 1u);
        }
    } else if (a == n) keep[a] = 0u;
    const unsigned lane = threadIdx.x & 63;
    const u64 bs = __ballot(split), bp = __ballot(split_passed);
    if (bs && lane == (unsigned)__builtin_ctzll(bs)) atomicAdd(&ctr[IN_SPLIT], (u64)__builtin_popcountll(bs));
    if (bp && lane == (unsigned)__builtin_ctzll(bp)) atomicAdd(&ctr[IN_SPLIT_PASSED], (u64)__builtin_popcountll(bp));
}

__global__ __launch_bounds__(IN_THREADS) void k_in_reads(const uint32_t *sel, const uint32_t *first, const int64_t *boff, const uint32_t *len, const uint64_t *src_off, int64_t M,
                                                         int64_t *old_of_new, uint32_t *nlen, uint64_t *noff, uint64_t *srcb)
{
    const int64_t v = (int64_t)blockIdx.x * IN_THREADS + threadIdx.x;
    if (v >= M || !sel[v]) return;
    const uint32_t w = first[v];
    old_of_new[w] = v;
    if (len) { nlen[w] = len[v]; noff[w] = (uint64_t)boff[v]; srcb[w] = 4 * src_off[v]; }
}

__global__ __launch_bounds__(IN_THREADS) void k_in_pairs_scatter(const int64_t *rows, const int64_t *cols, const elba_overlap_t *vals, int64_t n, const uint32_t *keep,
                                                                 const uint32_t *pos, const uint32_t *first, int64_t *orow, int64_t *ocol, elba_overlap_t *oval)
{
    static_assert(sizeof(elba_overlap_t) == 36 && alignof(elba_overlap_t) == 4, "the record is copied as nine dwords");
    const int64_t a = (int64_t)blockIdx.x * IN_THREADS + threadIdx.x;
    if (a >= n || !keep[a]) return;
    const uint32_t at = pos[a];
    orow[at] = (int64_t)first[rows[a]]; ocol[at] = (int64_t)first[cols[a]];      // (both ends selected: below M, checked by the mark)
    const uint32_t *s = reinterpret_cast<const uint32_t *>(vals + a);
    uint32_t *d = reinterpret_cast<uint32_t *>(oval + at);
    uint32_t t[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) t[i] = s[i];
#pragma unroll
    for (int i = 0; i < 9; ++i) d[i] = t[i];
}

inline unsigned in_blocks(int64_t lanes) { return (unsigned)((lanes + IN_THREADS - 1) / IN_THREADS); }

template <class T>
T *in_host_copy(Ctx &c, const DevBuf &b, size_t n)
{
    T *p = host_block<T>(n);
    copy_out(c, p, b.p, n);
    return p;
}

}  // namespace

void stage_induce_part(Ctx &c, const elba_induce_cfg *cfg, const int32_t *part_of_read, int64_t nreads, elba_induced_t *out)
{
    ELBA_REQUIRE(cfg && out && part_of_read, ELBA_ERR_INVALID_ARG, "induce_part: null cfg, output or part_of_read");
    ELBA_REQUIRE((cfg->flags & ~(ELBA_INDUCE_BASES | ELBA_INDUCE_HOST)) == 0, ELBA_ERR_INVALID_ARG, "induce_part: unknown flag");
    ELBA_REQUIRE(cfg->reserved[0] == 0 && cfg->reserved[1] == 0, ELBA_ERR_INVALID_ARG, "induce_part: non-zero reserved word");
    const GraphInput in = graph_input(c, "induce_part");
    const int64_t M = in.M, n = in.n;
    ELBA_REQUIRE(nreads == M, ELBA_ERR_INVALID_ARG, "induce_part: need one entry of part_of_read per read of the graph's input");
    const bool bases = (cfg->flags & ELBA_INDUCE_BASES) != 0, host = (cfg->flags & ELBA_INDUCE_HOST) != 0;
    ReadSource src{};
    if (bases) src = read_source(c, M, "induce_part", "bases of the graph's # reads", in.id_base == 0);
    ELBA_REQUIRE(M < 0x7fffffffll && M + in.id_base < 0xFFFFFFFFll, ELBA_ERR_UNSUPPORTED, "induce_part: read ids beyond 32 bit");
    ELBA_REQUIRE(n < 0x7fffffffll, ELBA_ERR_UNSUPPORTED, "induce_part: more than 2^31 pairs");

    hipStream_t s = c.stream;
    Ctx::InduceStage &k = c.in;
    k.part.reserve((size_t)(M + 1) * 4); k.sel.reserve((size_t)(M + 1) * 4); k.bytes.reserve((size_t)(M + 1) * 4); k.first.reserve((size_t)(M + 1) * 4);
    k.boff.reserve((size_t)(M + 1) * 8); k.oa.reserve((size_t)(M + 1) * 4); k.op.reserve((size_t)(M + 1) * 4);
    k.keep.reserve((size_t)(n + 1) * 4); k.pos.reserve((size_t)(n + 1) * 4); k.ctr.reserve(IN_CTR * 8);
    c.ws_scan.reserve((size_t)(((M > n ? M : n) + 1) / 1024 + 64) * 8);
    uint32_t *sel = k.sel.as<uint32_t>(), *bytes = k.bytes.as<uint32_t>(), *first = k.first.as<uint32_t>(), *keep = k.keep.as<uint32_t>(), *pos = k.pos.as<uint32_t>();
    uint32_t *oa = k.oa.as<uint32_t>(), *op = k.op.as<uint32_t>();
    int64_t *boff = k.boff.as<int64_t>();
    u64 *ctr = k.ctr.as<u64>();

    k.t_total.start(s);
    if (M > 0) ELBA_HIP(hipMemcpyAsync(k.part.p, part_of_read, (size_t)M * 4, hipMemcpyHostToDevice, s));
    ELBA_HIP(hipMemsetAsync(ctr, 0, IN_CTR * 8, s));
    ELBA_HIP(hipMemsetAsync(oa, 0, (size_t)(M + 1) * 4, s));
    ELBA_HIP(hipMemsetAsync(op, 0, (size_t)(M + 1) * 4, s));
    hipLaunchKernelGGL(k_in_select, dim3(in_blocks(M + 1)), dim3(IN_THREADS), 0, s, k.part.as<int32_t>(), cfg->part, bases ? src.len : nullptr, M, sel, bytes, ctr);
    exclusive_scan_u32(s, sel, first, M + 1, c.ws_scan);
    exclusive_scan_u32_to_i64(s, bytes, boff, M + 1, c.ws_scan);
    k.t_pairs.start(s);
    hipLaunchKernelGGL(k_in_pairs_mark, dim3(in_blocks(n + 1)), dim3(IN_THREADS), 0, s, in.rows, in.cols, in.vals, n, M, sel, first, keep, oa, op, ctr);
    exclusive_scan_u32(s, keep, pos, n + 1, c.ws_scan);
    k.t_pairs.stop(s);
    ELBA_HIP(hipGetLastError());
    uint32_t reads32 = 0, pairs32 = 0;
    int64_t pb = 0;
    ELBA_HIP(hipMemcpyAsync(&reads32, first + M, 4, hipMemcpyDeviceToHost, s));
    ELBA_HIP(hipMemcpyAsync(&pairs32, pos + n, 4, hipMemcpyDeviceToHost, s));
    ELBA_HIP(hipMemcpyAsync(&pb, boff + M, 8, hipMemcpyDeviceToHost, s));
    ELBA_HIP(hipStreamSynchronize(s));
    const int64_t R = (int64_t)reads32, P = (int64_t)pairs32;
    ELBA_REQUIRE(R <= M && P <= n && pb >= 0 && (bases || pb == 0), ELBA_ERR_INTERNAL, "induce_part: the scanned flags are not a selection");

    k.old_of_new.reserve((size_t)(R + 1) * 8);
    k.rows.reserve((size_t)(P + 1) * 8); k.cols.reserve((size_t)(P + 1) * 8); k.vals.reserve((size_t)(P + 1) * sizeof(elba_overlap_t));
    if (bases) { k.packed.reserve((size_t)pb + 16); k.off.reserve((size_t)(R + 1) * 8); k.len.reserve((size_t)(R + 1) * 4); k.srcb.reserve((size_t)(R + 1) * 8); }
    if (M > 0)
        hipLaunchKernelGGL(k_in_reads, dim3(in_blocks(M)), dim3(IN_THREADS), 0, s, sel, first, boff, bases ? src.len : nullptr, bases ? src.byte_off : nullptr, M,
                           k.old_of_new.as<int64_t>(), k.len.as<uint32_t>(), k.off.as<uint64_t>(), k.srcb.as<uint64_t>());
    k.t_scatter.start(s);
    if (P > 0)
        hipLaunchKernelGGL(k_in_pairs_scatter, dim3(in_blocks(n)), dim3(IN_THREADS), 0, s, in.rows, in.cols, in.vals, n, keep, pos, first, k.rows.as<int64_t>(),
                           k.cols.as<int64_t>(), k.vals.as<elba_overlap_t>());
    k.t_scatter.stop(s);
    k.t_gather.start(s);
    if (bases) {
        // the last word's tail and the guard bytes; the words below are written whole by the kernel
        ELBA_HIP(hipMemsetAsync(k.packed.as<uint8_t>() + (pb & ~7ll), 0, (size_t)(pb - (pb & ~7ll)) + 16, s));
        if (pb > 0) {
            const int64_t nwords = (pb + 7) / 8;
            ELBA_REQUIRE((nwords + TRIM_THREADS - 1) / TRIM_THREADS < 0x7fffffffll, ELBA_ERR_UNSUPPORTED, "induce_part: more than 2^42 packed bytes");
            hipLaunchKernelGGL(k_trim_repack, dim3((unsigned)((nwords + TRIM_THREADS - 1) / TRIM_THREADS)), dim3(TRIM_THREADS), 0, s, src.packed, k.off.as<uint64_t>(),
                               k.len.as<uint32_t>(), k.srcb.as<uint64_t>(), R, (uint64_t)pb, k.packed.as<uint64_t>());
        }
    }
    k.t_gather.stop(s);
    ELBA_HIP(hipGetLastError());
    k.t_total.stop(s);
    u64 h[IN_CTR] = {0};
    ELBA_HIP(hipMemcpyAsync(h, ctr, IN_CTR * 8, hipMemcpyDeviceToHost, s));
    ELBA_HIP(hipStreamSynchronize(s));

    elba_induced_t o{};
    o.reads = R; o.pairs = P; o.packed_bytes = bases ? pb : 0;
    o.d_old_of_new = k.old_of_new.p; o.d_rows = k.rows.p; o.d_cols = k.cols.p; o.d_vals = k.vals.p; o.d_outside_aligned = oa; o.d_outside_passed = op;
    if (bases) { o.d_packed = k.packed.p; o.d_byte_off = k.off.p; o.d_len = k.len.p; }
    if (host) {
        *out = o;                                                   // (published as they are allocated: elba_free_induced releases them if a later step fails)
        out->old_of_new = in_host_copy<int64_t>(c, k.old_of_new, (size_t)R);
        out->rows = in_host_copy<int64_t>(c, k.rows, (size_t)P); out->cols = in_host_copy<int64_t>(c, k.cols, (size_t)P);
        out->vals = in_host_copy<elba_overlap_t>(c, k.vals, (size_t)P);
        out->outside_aligned = in_host_copy<uint32_t>(c, k.oa, (size_t)R); out->outside_passed = in_host_copy<uint32_t>(c, k.op, (size_t)R);
        if (bases) {
            out->packed = in_host_copy<uint8_t>(c, k.packed, (size_t)pb + 16);
            out->byte_off = in_host_copy<uint64_t>(c, k.off, (size_t)R); out->len = in_host_copy<uint32_t>(c, k.len, (size_t)R);
        }
        ELBA_HIP(hipStreamSynchronize(s));
    } else *out = o;

    elba_induce_stats st{};
    st.nreads_in = M; st.pairs_in = n; st.reads = R; st.pairs = P; st.bases = (int64_t)h[IN_BASES]; st.packed_bytes = o.packed_bytes;
    st.split_pairs = (int64_t)h[IN_SPLIT]; st.split_passed = (int64_t)h[IN_SPLIT_PASSED]; st.id_base = in.id_base;
    st.ms_total = k.t_total.ms(); st.ms_pairs = k.t_pairs.ms() + k.t_scatter.ms(); st.ms_gather = k.t_gather.ms();
    k.stats = st;
}

}  // namespace elba
