// trim.hip — the reads cut to their supported intervals: what PileupVector::GetTrimmedInterval's [beststart, bestend] is computed for
// (src/PruneChimeras.cpp:31-69; main.cpp never calls that file, so the reference never cuts).  elba_trim_reads turns the last pileup's
// intervals back into a read set in DnaBuffer layout that the pipeline runs on again: reads -> pileup -> pieces -> k-mers -> ... -> contigs.
//
// mode 0: one piece per read, its trimmed interval [trim_beg, trim_end); mode 1: one piece per long run, a maximal run of depth >= min_depth
// at least min_run bases long (the runs k_pu_reads counts for the flags, min_depth / min_run of the pileup's own cfg).  A piece shorter than
// min_len is dropped.  Pieces are numbered by (src_read, src_beg) ascending.
//
//   k_trim_count    one lane per read over its trim pair / its segments: pieces passing min_len, their packed bytes, the stats (one atomic
//                   per wavefront and counter)
//   scans           cnt -> first piece of every read (u32), bytes -> first output byte of every read (i64)
//   -- the one host synchronisation: the piece count n and packed_bytes (they size the output) and the other counters --
//   k_trim_pieces   the same walk: (src_read, beg, end), byte_off, len of every piece, and srcb[p] = the piece's first base counted from
//                   the start of the source buffer (4 x the read's byte offset + beg)
//   k_trim_repack   (repack.hpp, shared with induce.hip) flat over the OUTPUT: a lane owns one aligned 8-byte word.  Pieces are byte-aligned and lie back to back (byte_off is
//                   the running sum of (len + 3) / 4), so every byte of a word below packed_bytes belongs to exactly one piece and the lane
//                   writes its word whole, in one store — never a neighbour's byte.  A word inside one piece (all but two words of a long
//                   piece) takes two aligned 8-byte source loads; a word with piece boundaries in it walks its pieces (at most 8: a piece
//                   has at least one byte).  Bases are big-endian inside a byte (src/DnaSeq.cpp:17), so the two source words are
//                   byte-swapped, funnel-shifted left by 8 x (source byte mod 8) + 2 x (beg mod 4) bits and swapped back.  The unused low
//                   bits of a piece's last byte are masked to zero whatever follows in the source.  The workgroup's first and last piece
//                   are found by two binary searches of byte_off (two lanes), a lane then searches between them: 0 or 1 steps where a
//                   workgroup's 2 KiB lie in one or two pieces, log2(2048) at the worst.  No LDS beyond those two indices, no scratch.
//
// Bounds.  Reads r < M, pieces p < n, cnt / bytes / first / boff have M + 1 entries, the per-piece arrays n + 1.  Output: words
// w < ceil(packed_bytes / 8); the buffer holds packed_bytes + 16 and the bytes from packed_bytes & ~7 on are zeroed before the kernel, so
// the last word's tail and the 16 guard bytes are zero.  Source: output byte j of piece p comes from source bytes s and s + 1 with
// s = off[r] + beg / 4 + j <= off[r] + (end - 1) / 4 < packed_bytes(source); the aligned words at s & ~7 and (s & ~7) + 8 end at most at
// s + 15 < packed_bytes(source) + 15: inside the 16 guard bytes every read buffer of a context carries.
// Bytes moved (algorithmic): bases_out / 4 read, bases_out / 4 written, 16 B per piece (byte_off + srcb; len where a piece ends), the
// segment walk twice (12 B per segment of mode 1, 8 B per read of mode 0) and 28 B per piece written by k_trim_pieces.
#include "common.hpp"
#include "repack.hpp"      // k_trim_repack, trim_find, TRIM_THREADS: shared with induce.hip

namespace elba {

namespace {

struct TrimParams {
    const int64_t *seg_off; const int32_t *seg_start, *seg_depth; const int2 *trim;
    const uint32_t *len; const uint64_t *src_off; uint32_t M;
    int mode, min_depth, min_run, min_len;
};

// the pieces of read r in ascending order: emit(beg, end)
template <class F>
__device__ __forceinline__ void trim_walk(const TrimParams &p, uint32_t r, F &&emit)
{
    if (p.mode == 0) {
        const int2 t = p.trim[r];
        if (t.x >= 0 && t.y - t.x >= p.min_len) emit(t.x, t.y);
        return;
    }
    const int64_t s0 = p.seg_off[r], s1 = p.seg_off[r + 1];
    const int32_t L = (int32_t)p.len[r];
    int32_t start = -1;
    for (int64_t j = s0; j < s1; ++j) {
        if (p.seg_depth[j] >= p.min_depth) { if (start < 0) start = p.seg_start[j]; continue; }
        if (start >= 0) {
            const int32_t a = p.seg_start[j];
            if (a - start >= p.min_run && a - start >= p.min_len) emit(start, a);
            start = -1;
        }
    }
    if (start >= 0 && L - start >= p.min_run && L - start >= p.min_len) emit(start, L);
}

__device__ __forceinline__ unsigned long long wave_add(unsigned long long v)
{
    for (int o = 32; o >= 1; o >>= 1) v += (unsigned long long)__shfl_xor((long long)v, o);
    return v;
}

// ctr: 0 pieces, 1 reads without a piece, 2 reads with two or more, 3 reads whose one piece is [0, len), 4 bases in, 5 bases out, 6 packed bytes, 7 longest piece
__global__ void k_trim_count(TrimParams p, uint32_t *cnt, uint32_t *bytes, unsigned long long *ctr)
{
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long n = 0, nb = 0, bases = 0, lin = 0, longest = 0;
    bool dropped = false, split = false, same = false;
    if (r < p.M) {
        const int32_t L = (int32_t)p.len[r];
        bool whole = false;
        trim_walk(p, r, [&](int32_t b, int32_t e) {
            const unsigned long long l = (unsigned long long)(e - b);
            ++n; nb += (l + 3) >> 2; bases += l; longest = l > longest ? l : longest;
            whole = b == 0 && e == L;
        });
        cnt[r] = (uint32_t)n; bytes[r] = (uint32_t)nb;
        lin = (unsigned long long)L;
        dropped = n == 0; split = n >= 2; same = n == 1 && whole;
    } else if (r == p.M) { cnt[r] = 0; bytes[r] = 0; }
    const unsigned long long nd = (unsigned long long)__builtin_popcountll(__ballot(dropped)), ns = (unsigned long long)__builtin_popcountll(__ballot(split)),
                             nu = (unsigned long long)__builtin_popcountll(__ballot(same));
    n = wave_add(n); nb = wave_add(nb); bases = wave_add(bases); lin = wave_add(lin);
    for (int o = 32; o >= 1; o >>= 1) { const unsigned long long w = (unsigned long long)__shfl_xor((long long)longest, o); longest = w > longest ? w : longest; }
    if ((threadIdx.x & 63) == 0) {
        if (n) atomicAdd(&ctr[0], n);
        if (nd) atomicAdd(&ctr[1], nd);
        if (ns) atomicAdd(&ctr[2], ns);
        if (nu) atomicAdd(&ctr[3], nu);
        if (lin) atomicAdd(&ctr[4], lin);
        if (bases) atomicAdd(&ctr[5], bases);
        if (nb) atomicAdd(&ctr[6], nb);
        if (longest) atomicMax(&ctr[7], longest);
    }
}

__global__ void k_trim_pieces(TrimParams p, const uint32_t *first, const int64_t *boff, int64_t *src_read, int32_t *src_beg, int32_t *src_end, uint64_t *byte_off,
                              uint32_t *plen, uint64_t *srcb)
{
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= p.M) return;
    int64_t at = first[r];
    uint64_t bo = (uint64_t)boff[r];
    const uint64_t sbase = 4 * p.src_off[r];
    trim_walk(p, r, [&](int32_t b, int32_t e) {
        src_read[at] = r; src_beg[at] = b; src_end[at] = e;
        byte_off[at] = bo; plen[at] = (uint32_t)(e - b); srcb[at] = sbase + (uint64_t)b;
        bo += (uint64_t)(e - b + 3) >> 2; ++at;
    });
}

}  // namespace

void stage_trim_reads(Ctx &c, const elba_trim_cfg *cfgp)
{
    enter(c.v, EV_TRIM_READS);
    ELBA_REQUIRE(cfgp, ELBA_ERR_INVALID_ARG, "trim_reads: null cfg");
    const elba_trim_cfg &cfg = *cfgp;
    ELBA_REQUIRE(cfg.mode == 0 || cfg.mode == 1, ELBA_ERR_INVALID_ARG, "trim_reads: mode must be 0 (trimmed intervals) or 1 (long runs)");
    ELBA_REQUIRE(cfg.min_len >= 1, ELBA_ERR_INVALID_ARG, "trim_reads: need min_len >= 1");
    ELBA_REQUIRE(cfg.reserved[0] == 0 && cfg.reserved[1] == 0, ELBA_ERR_INVALID_ARG, "trim_reads: reserved words must be 0");
    ELBA_REQUIRE(has(c.v, P_PILEUP), ELBA_ERR_STATE, "trim_reads: no pileup of the current overlaps (call elba_read_pileup)");
    const int64_t M = c.pu.M;
    const ReadSource in = read_source(c, M, "trim_reads", "bases of the pileup's # reads");
    accepted(c.v, EV_TRIM_READS);
    hipStream_t s = c.stream;
    TrimParams p{};
    p.seg_off = c.pu.depth.seg_off.as<int64_t>(); p.seg_start = c.pu.depth.seg_start.as<int32_t>(); p.seg_depth = c.pu.depth.seg_depth.as<int32_t>(); p.trim = c.pu.trim.as<int2>();
    p.len = in.len; p.src_off = in.byte_off; p.M = (uint32_t)M;
    p.mode = cfg.mode; p.min_depth = c.pu.cfg.min_depth; p.min_run = c.pu.cfg.min_run; p.min_len = cfg.min_len;
    c.tm.cnt.reserve((size_t)(M + 1) * 4); c.tm.bytes.reserve((size_t)(M + 1) * 4); c.tm.first.reserve((size_t)(M + 1) * 4); c.tm.boff.reserve((size_t)(M + 1) * 8);
    c.tm.ctr.reserve(64);
    uint32_t *cnt = c.tm.cnt.as<uint32_t>(), *bytes = c.tm.bytes.as<uint32_t>(), *first = c.tm.first.as<uint32_t>();
    int64_t *boff = c.tm.boff.as<int64_t>();
    unsigned long long *ctr = c.tm.ctr.as<unsigned long long>();
    const unsigned nbM = (unsigned)((M + 1 + 255) / 256);
    c.tm.t_total.start(s);
    ELBA_HIP(hipMemsetAsync(ctr, 0, 64, s));
    hipLaunchKernelGGL(k_trim_count, dim3(nbM), dim3(256), 0, s, p, cnt, bytes, ctr);
    exclusive_scan_u32(s, cnt, first, M + 1, c.ws_scan);
    exclusive_scan_u32_to_i64(s, bytes, boff, M + 1, c.ws_scan);
    ELBA_HIP(hipGetLastError());
    unsigned long long h[8] = {0};
    ELBA_HIP(hipMemcpyAsync(h, ctr, 64, hipMemcpyDeviceToHost, s));
    ELBA_HIP(hipStreamSynchronize(s));
    const int64_t n = (int64_t)h[0], pb = (int64_t)h[6];
    c.tm.packed.reserve((size_t)pb + 16); c.tm.off.reserve((size_t)(n + 1) * 8); c.tm.len.reserve((size_t)(n + 1) * 4);
    c.tm.src.reserve((size_t)(n + 1) * 8); c.tm.beg.reserve((size_t)(n + 1) * 4); c.tm.end.reserve((size_t)(n + 1) * 4); c.tm.srcb.reserve((size_t)(n + 1) * 8);
    if (M > 0)
        hipLaunchKernelGGL(k_trim_pieces, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, p, first, boff, c.tm.src.as<int64_t>(), c.tm.beg.as<int32_t>(),
                           c.tm.end.as<int32_t>(), c.tm.off.as<uint64_t>(), c.tm.len.as<uint32_t>(), c.tm.srcb.as<uint64_t>());
    // the last word's tail and the guard bytes; the words below are written whole by the kernel
    ELBA_HIP(hipMemsetAsync(c.tm.packed.as<uint8_t>() + (pb & ~7ll), 0, (size_t)(pb - (pb & ~7ll)) + 16, s));
    c.tm.t_repack.start(s);
    if (n > 0) {
        const int64_t nwords = (pb + 7) / 8;
        ELBA_REQUIRE((nwords + TRIM_THREADS - 1) / TRIM_THREADS < 0x7fffffffll, ELBA_ERR_UNSUPPORTED, "trim_reads: more than 2^42 packed bytes");
        hipLaunchKernelGGL(k_trim_repack, dim3((unsigned)((nwords + TRIM_THREADS - 1) / TRIM_THREADS)), dim3(TRIM_THREADS), 0, s, in.packed, c.tm.off.as<uint64_t>(),
                           c.tm.len.as<uint32_t>(), c.tm.srcb.as<uint64_t>(), n, (uint64_t)pb, c.tm.packed.as<uint64_t>());
    }
    c.tm.t_repack.stop(s);
    ELBA_HIP(hipGetLastError());
    c.tm.t_total.stop(s);
    ELBA_HIP(hipStreamSynchronize(s));
    elba_trim_stats st{};
    st.nreads_in = M; st.pieces = n; st.reads_dropped = (int64_t)h[1]; st.reads_split = (int64_t)h[2]; st.reads_unchanged = (int64_t)h[3];
    st.bases_in = (int64_t)h[4]; st.bases_out = (int64_t)h[5]; st.packed_bytes = pb; st.longest = (int64_t)h[7];
    st.ms_total = c.tm.t_total.ms(); st.ms_repack = c.tm.t_repack.ms();
    c.tm.n = n; c.tm.packed_bytes = pb; c.tm.stats = st; done(c.v, EV_TRIM_READS);
}

// the pieces become the context's own reads, exactly as after elba_set_reads
void stage_adopt_trimmed_reads(Ctx &c)
{
    ELBA_REQUIRE(has(c.v, P_TRIM), ELBA_ERR_STATE, "adopt_trimmed_reads: no trimmed reads (call elba_trim_reads)");
    hipStream_t s = c.stream;
    const int64_t n = c.tm.n;
    std::vector<uint32_t> hl((size_t)n);
    std::vector<uint64_t> ho((size_t)n);
    if (n) {
        ELBA_HIP(hipMemcpyAsync(hl.data(), c.tm.len.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
        ELBA_HIP(hipMemcpyAsync(ho.data(), c.tm.off.p, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    }
    ELBA_HIP(hipStreamSynchronize(s));
    c.own_packed.swap(c.tm.packed); c.own_byte_off.swap(c.tm.off); c.own_len.swap(c.tm.len);
    c.d_packed = c.own_packed.as<uint8_t>(); c.d_byte_off = c.own_byte_off.as<uint64_t>(); c.d_len = c.own_len.as<uint32_t>();
    c.h_len.swap(hl); c.h_byte_off.swap(ho);
    c.nreads = n; c.first_global_id = 0; c.packed_bytes = c.tm.packed_bytes;
    reads_replaced(c, EV_ADOPT_TRIMMED_READS);
}

}  // namespace elba
