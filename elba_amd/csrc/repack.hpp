// repack.hpp — the 2-bit gather that trim.hip (pieces of reads) and induce.hip (whole reads, beg = 0) share: k_trim_repack and the binary
// search it stands on.  What the kernel does, its bounds and its bytes are written down in trim.hip's header; both stages include this file,
// so there is one copy of the kernel's text (each translation unit compiles its own code object from it, as with sg_rounds.hpp).
//
// The caller's side of the contract: byte_off[0 .. n) ascending from 0 with byte_off[p + 1] - byte_off[p] = (plen[p] + 3) / 4, srcb[p] = the
// piece's first base counted from the start of src (srcb[p] / 4 <= the source's packed bytes), src followed by 16 readable guard bytes, out
// holding ceil(packed_bytes / 8) words, n >= 1, packed_bytes >= 1, grid = ceil(ceil(packed_bytes / 8) / TRIM_THREADS).
// A piece of 0 bases (trim.hip has none, induce.hip has a read of length 0) has no byte and shares its offset with its successor.  It is
// harmless: trim_find returns the LAST piece at or below a byte, which among pieces of one offset is the one that owns bytes (pieces of 0
// bases behind the last byte stand at packed_bytes, above every byte looked up), and the walk through a word meets such a piece only
// behind a piece that owns bytes of the word, with 1 <= lo = hi <= 7: its mask is empty and it adds nothing.
#pragma once
#include "common.hpp"

namespace elba {

namespace {

constexpr int TRIM_THREADS = 256;

// last piece p in [lo, hi] with byte_off[p] <= x (byte_off[lo] <= x)
__device__ __forceinline__ int64_t trim_find(const uint64_t *byte_off, int64_t lo, int64_t hi, uint64_t x)
{
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (byte_off[mid] <= x) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(TRIM_THREADS) void k_trim_repack(const uint8_t *__restrict__ src, const uint64_t *__restrict__ byte_off, const uint32_t *__restrict__ plen,
                                                              const uint64_t *__restrict__ srcb, int64_t n, uint64_t packed_bytes, uint64_t *__restrict__ out)
{
    __shared__ int64_t span[2];
    const uint64_t nwords = (packed_bytes + 7) >> 3;
    const uint64_t wb = (uint64_t)blockIdx.x * TRIM_THREADS;                 // the workgroup's first word (< nwords: the grid is ceil(nwords / 256))
    if (threadIdx.x == 0) span[0] = trim_find(byte_off, 0, n - 1, wb << 3);
    if (threadIdx.x == 64) {
        uint64_t last = ((wb + TRIM_THREADS) << 3) - 1;
        if (last >= packed_bytes) last = packed_bytes - 1;
        span[1] = trim_find(byte_off, 0, n - 1, last);
    }
    __syncthreads();
    const uint64_t w = wb + threadIdx.x;
    if (w >= nwords) return;
    const uint64_t o0 = w << 3;                                              // first output byte of the word (< packed_bytes)
    int64_t p = trim_find(byte_off, span[0], span[1], o0);
    uint64_t W = 0;                                                          // the word, big-endian: output byte 0 in bits 63..56
    uint64_t pbeg = byte_off[p];
    for (;;) {
        const uint64_t pend = p + 1 < n ? byte_off[p + 1] : packed_bytes;    // the piece's bytes are [pbeg, pend)
        const uint32_t lo = pbeg > o0 ? (uint32_t)(pbeg - o0) : 0u;          // bytes [lo, hi) of the word are this piece's
        const bool ends = pend <= o0 + 8;
        const uint32_t hi = ends ? (uint32_t)(pend - o0) : 8u;
        const uint64_t sb = srcb[p];
        const uint64_t s = (sb >> 2) + (o0 + lo - pbeg);                     // source byte holding the first base of output byte o0 + lo
        const uint64_t *a = reinterpret_cast<const uint64_t *>(src + (s & ~7ull));
        const uint64_t x = __builtin_bswap64(a[0]), y = __builtin_bswap64(a[1]);
        const uint32_t t = (uint32_t)(s & 7) * 8 + (uint32_t)(sb & 3) * 2;  // 0 .. 62
        const uint64_t v = t ? (x << t) | (y >> (64 - t)) : x;
        uint32_t cut = 64 - 8 * hi;                                          // bits below `cut` are not this piece's
        if (ends) cut += 2 * (4 * (uint32_t)(pend - pbeg) - plen[p]);        // ... nor the unused low bits of its last byte
        W |= (v >> (8 * lo)) & (~0ull >> (8 * lo)) & (~0ull << cut);
        if (pend >= o0 + 8 || pend >= packed_bytes) break;                   // the word is full (a piece that ends with it included), or the buffer ends
        ++p; pbeg = pend;
    }
    out[w] = __builtin_bswap64(W);
}

}  // namespace

}  // namespace elba
