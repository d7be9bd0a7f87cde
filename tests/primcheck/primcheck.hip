// primcheck.hip — a test-only harness over the device primitives of prims.hip (tests/test_gpu_primitives.py).  NOT part of the product
// ABI: it calls the internal functions that common.hpp declares and libelba_amd.so happens to export, and is never loaded by elba_amd.
//
// Every entry takes HOST arrays, copies them into device buffers of its own, calls ONE primitive on the null stream with a workspace of its
// own, synchronises, asks hipGetLastError, copies the results back and returns an elba status; an ELBA_REQUIRE or a failed HIP call comes
// back as that status (primcheck_last_error has the text), never as an exception.  No kernel lives here.
//
// Two safeguards, both on the host: (1) arguments with which a primitive would write outside its output (keys that are not ascending for
// the group offsets, a read id >= M in a CSR key, a handed-over histogram that is not the keys' own) are refused with ELBA_ERR_INVALID_ARG
// before anything is launched; (2) every device buffer carries 256 guard bytes behind its payload, checked after the call: a primitive
// that wrote beyond its output comes back as ELBA_ERR_INTERNAL.
#include "../../elba_amd/csrc/common.hpp"

#include <algorithm>

namespace {

using elba::DevBuf;
using elba::Error;

thread_local std::string g_err;

constexpr size_t GUARD = 256;
constexpr uint8_t GUARD_BYTE = 0xA5;

// a device buffer of `bytes` payload bytes + GUARD guard bytes
struct Dev {
    DevBuf b;
    size_t bytes = 0;
    void alloc(size_t n)
    {
        bytes = n;
        b.reserve_exact(n + GUARD);
        ELBA_HIP(hipMemset(static_cast<uint8_t *>(b.p) + n, GUARD_BYTE, GUARD));
    }
    void upload(const void *host, size_t n)
    {
        alloc(n);
        if (n) ELBA_HIP(hipMemcpy(b.p, host, n, hipMemcpyHostToDevice));
    }
    void download(void *host, const char *what)
    {
        uint8_t g[GUARD];
        ELBA_HIP(hipMemcpy(g, static_cast<uint8_t *>(b.p) + bytes, GUARD, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < GUARD; ++i)
            ELBA_REQUIRE(g[i] == GUARD_BYTE, ELBA_ERR_INTERNAL, std::string("primcheck: guard bytes behind ") + what + " were overwritten");
        if (bytes) ELBA_HIP(hipMemcpy(host, b.p, bytes, hipMemcpyDeviceToHost));
    }
    template <class T> T *as() const { return b.as<T>(); }
};

void finish()
{
    ELBA_HIP(hipDeviceSynchronize());
    ELBA_HIP(hipGetLastError());
}

template <class F> int guarded(F &&f)
{
    try {
        g_err.clear();
        f();
        return ELBA_OK;
    } catch (const Error &e) {
        g_err = e.msg;
        (void)hipGetLastError();
        return e.code;
    } catch (const std::exception &e) {
        g_err = e.what();
        return ELBA_ERR_INTERNAL;
    }
}

void require_bits(int bit_lo, int bit_hi, int maxbit)
{
    ELBA_REQUIRE(bit_lo >= 0 && bit_lo <= maxbit && bit_hi >= 0 && bit_hi <= maxbit, ELBA_ERR_INVALID_ARG, "primcheck: sort bits outside the key");
}

template <class K> void require_ascending(const K *keys, int shift, int64_t n, int64_t nkeys)
{
    ELBA_REQUIRE(n >= 0 && nkeys >= 0 && shift >= 0 && shift < (int)(8 * sizeof(K)), ELBA_ERR_INVALID_ARG, "primcheck: group offsets: bad sizes");
    for (int64_t z = 0; z < n; ++z) {
        ELBA_REQUIRE((uint64_t)(keys[z] >> shift) <= (uint64_t)nkeys, ELBA_ERR_INVALID_ARG, "primcheck: group offsets: a key behind nkeys");
        ELBA_REQUIRE(z == 0 || (keys[z - 1] >> shift) <= (keys[z] >> shift), ELBA_ERR_INVALID_ARG, "primcheck: group offsets: keys not ascending");
    }
}

}  // namespace

extern "C" {

const char *primcheck_last_error() { return g_err.c_str(); }

// out[0 .. n) = exclusive prefix sums of in (mod 2^32).  inplace != 0: the scan runs with in == out.
int primcheck_exclusive_scan_u32(const uint32_t *in, uint32_t *out, int64_t n, int inplace)
{
    return guarded([&] {
        ELBA_REQUIRE(n >= 0, ELBA_ERR_INVALID_ARG, "primcheck: n < 0");
        Dev di, dout; DevBuf tmp;
        di.upload(in, (size_t)n * 4);
        if (!inplace) dout.upload(out, (size_t)n * 4);
        elba::exclusive_scan_u32(nullptr, di.as<uint32_t>(), inplace ? di.as<uint32_t>() : dout.as<uint32_t>(), n, tmp);
        finish();
        (inplace ? di : dout).download(out, "the scan's output");
    });
}

int primcheck_exclusive_scan_u32_to_i64(const uint32_t *in, int64_t *out, int64_t n)
{
    return guarded([&] {
        ELBA_REQUIRE(n >= 0, ELBA_ERR_INVALID_ARG, "primcheck: n < 0");
        Dev di, dout; DevBuf tmp;
        di.upload(in, (size_t)n * 4);
        dout.upload(out, (size_t)n * 8);
        elba::exclusive_scan_u32_to_i64(nullptr, di.as<uint32_t>(), dout.as<int64_t>(), n, tmp);
        finish();
        dout.download(out, "the scan's output");
    });
}

int primcheck_fill_u32(uint32_t *buf, int64_t total, uint32_t v, int64_t n)      // buf[0 .. total): in and out, the first n are filled
{
    return guarded([&] {
        ELBA_REQUIRE(total >= 0 && n <= total, ELBA_ERR_INVALID_ARG, "primcheck: fill beyond the buffer");
        Dev d;
        d.upload(buf, (size_t)total * 4);
        elba::fill_u32(nullptr, d.as<uint32_t>(), v, n);
        finish();
        d.download(buf, "the filled buffer");
    });
}

int primcheck_fill_u64(uint64_t *buf, int64_t total, uint64_t v, int64_t n)
{
    return guarded([&] {
        ELBA_REQUIRE(total >= 0 && n <= total, ELBA_ERR_INVALID_ARG, "primcheck: fill beyond the buffer");
        Dev d;
        d.upload(buf, (size_t)total * 8);
        elba::fill_u64(nullptr, d.as<uint64_t>(), v, n);
        finish();
        d.download(buf, "the filled buffer");
    });
}

int primcheck_reduce_max_u64(const uint64_t *in, int64_t n, uint64_t *out)
{
    return guarded([&] {
        ELBA_REQUIRE(n >= 0, ELBA_ERR_INVALID_ARG, "primcheck: n < 0");
        Dev d; DevBuf tmp;
        d.upload(in, (size_t)n * 8);
        *out = elba::reduce_max_u64(nullptr, d.as<uint64_t>(), n, tmp);
        finish();
    });
}

// ptr[0 .. nkeys]: in (whatever the caller wants to see survive) and out
int primcheck_group_offsets_u32(const uint64_t *keys, int key_shift, int64_t n, uint32_t *ptr, int64_t nkeys)
{
    return guarded([&] {
        require_ascending(keys, key_shift, n, nkeys);
        Dev dk, dp;
        dk.upload(keys, (size_t)n * 8);
        dp.upload(ptr, (size_t)(nkeys + 1) * 4);
        elba::group_offsets_u32(nullptr, dk.as<uint64_t>(), key_shift, n, dp.as<uint32_t>(), nkeys);
        finish();
        dp.download(ptr, "the group offsets");
    });
}

int primcheck_group_offsets_k32(const uint32_t *keys, int64_t n, uint32_t *ptr, int64_t nkeys)
{
    return guarded([&] {
        require_ascending(keys, 0, n, nkeys);
        Dev dk, dp;
        dk.upload(keys, (size_t)n * 4);
        dp.upload(ptr, (size_t)(nkeys + 1) * 4);
        elba::group_offsets_k32(nullptr, dk.as<uint32_t>(), n, dp.as<uint32_t>(), nkeys);
        finish();
        dp.download(ptr, "the group offsets");
    });
}

// rows[nrows][nbins]: in and out
int primcheck_radix_column_scan(uint32_t *rows, int64_t nrows, uint32_t nbins)
{
    return guarded([&] {
        ELBA_REQUIRE(nrows >= 1 && nbins >= 1 && nbins <= 1024, ELBA_ERR_INVALID_ARG, "primcheck: column scan: 1 <= nbins <= 1024 (one thread per column), nrows >= 1");
        Dev d; DevBuf tmp;
        d.upload(rows, (size_t)nrows * nbins * 4);
        elba::radix_column_scan(nullptr, d.as<uint32_t>(), nrows, nbins, tmp);
        finish();
        d.download(rows, "the histogram rows");
    });
}

int primcheck_radix_sort_where(int64_t n, int bit_lo, int bit_hi, int *where)      // (host code only)
{
    return guarded([&] { *where = elba::radix_sort_where(n, bit_lo, bit_hi); });
}

// Both buffer pairs are in and out: (k0, v0) holds the input, (k1, v1) whatever the caller wants to recognise afterwards; *where = what the sort returned.
int primcheck_radix_sort_pairs(uint64_t *k0, uint64_t *v0, uint64_t *k1, uint64_t *v1, int64_t n, int bit_lo, int bit_hi, int *where)
{
    return guarded([&] {
        ELBA_REQUIRE(n >= 0, ELBA_ERR_INVALID_ARG, "primcheck: n < 0");
        require_bits(bit_lo, bit_hi, 64);
        Dev a, b, c, d; DevBuf tmp;
        a.upload(k0, (size_t)n * 8); b.upload(v0, (size_t)n * 8); c.upload(k1, (size_t)n * 8); d.upload(v1, (size_t)n * 8);
        *where = elba::radix_sort_pairs(nullptr, a.as<uint64_t>(), b.as<uint64_t>(), c.as<uint64_t>(), d.as<uint64_t>(), n, bit_lo, bit_hi, tmp);
        finish();
        a.download(k0, "k0"); b.download(v0, "v0"); c.download(k1, "k1"); d.download(v1, "v1");
    });
}

int primcheck_radix_sort_pairs_k32(uint32_t *k0, uint64_t *v0, uint32_t *k1, uint64_t *v1, int64_t n, int bit_lo, int bit_hi, int *where)
{
    return guarded([&] {
        ELBA_REQUIRE(n >= 0, ELBA_ERR_INVALID_ARG, "primcheck: n < 0");
        require_bits(bit_lo, bit_hi, 32);
        Dev a, b, c, d; DevBuf tmp;
        a.upload(k0, (size_t)n * 4); b.upload(v0, (size_t)n * 8); c.upload(k1, (size_t)n * 4); d.upload(v1, (size_t)n * 8);
        *where = elba::radix_sort_pairs_k32(nullptr, a.as<uint32_t>(), b.as<uint64_t>(), c.as<uint32_t>(), d.as<uint64_t>(), n, bit_lo, bit_hi, tmp);
        finish();
        a.download(k0, "k0"); b.download(v0, "v0"); c.download(k1, "k1"); d.download(v1, "v1");
    });
}

int primcheck_radix_sort_keys(uint64_t *k0, uint64_t *k1, int64_t n, int bit_lo, int bit_hi, int *where)
{
    return guarded([&] {
        ELBA_REQUIRE(n >= 0, ELBA_ERR_INVALID_ARG, "primcheck: n < 0");
        require_bits(bit_lo, bit_hi, 64);
        Dev a, c; DevBuf tmp;
        a.upload(k0, (size_t)n * 8); c.upload(k1, (size_t)n * 8);
        *where = elba::radix_sort_keys(nullptr, a.as<uint64_t>(), c.as<uint64_t>(), n, bit_lo, bit_hi, tmp);
        finish();
        a.download(k0, "k0"); c.download(k1, "k1");
    });
}

// what radix_first_histogram tells a producer: the first pass's digit and the tile its rows of counts cover; *offset_bytes = where the rows start in the workspace
int primcheck_radix_first_histogram(int64_t n, int bit_lo, int bit_hi, int *shift, int *bits, int *tile, int64_t *offset_bytes)
{
    return guarded([&] {
        ELBA_REQUIRE(n >= 2 && bit_hi > bit_lo, ELBA_ERR_INVALID_ARG, "primcheck: first histogram of a sort that does not run");
        require_bits(bit_lo, bit_hi, 64);
        DevBuf tmp;
        uint32_t *h = elba::radix_first_histogram(n, bit_lo, bit_hi, tmp, shift, bits, tile);
        *offset_bytes = (int64_t)(reinterpret_cast<uint8_t *>(h) - static_cast<uint8_t *>(tmp.p));
    });
}

// radix_sort_keys with first_hist_done = true: counts[nrows][1 << bits] are the rows a producer counted (row t = the digit counts of the keys
// [t * tile, (t + 1) * tile)); they are placed where radix_first_histogram says.  Rows that are not the keys' own counts are refused: the
// scatter trusts them for its addresses.
int primcheck_radix_sort_keys_first_hist(uint64_t *k0, uint64_t *k1, int64_t n, int bit_lo, int bit_hi, const uint32_t *counts, int64_t nrows, int *where)
{
    return guarded([&] {
        ELBA_REQUIRE(n >= 2 && bit_hi > bit_lo, ELBA_ERR_INVALID_ARG, "primcheck: first histogram of a sort that does not run");
        require_bits(bit_lo, bit_hi, 64);
        Dev a, c; DevBuf tmp;
        int shift = 0, bits = 0, tile = 0;
        uint32_t *d_hist = elba::radix_first_histogram(n, bit_lo, bit_hi, tmp, &shift, &bits, &tile);
        const int64_t want_rows = (n + tile - 1) / tile;
        ELBA_REQUIRE(nrows == want_rows, ELBA_ERR_INVALID_ARG, "primcheck: first histogram: wrong number of rows");
        const size_t nbins = (size_t)1 << bits;
        std::vector<uint32_t> own((size_t)nrows * nbins, 0u);
        for (int64_t z = 0; z < n; ++z) ++own[(size_t)(z / tile) * nbins + (size_t)((k0[z] >> shift) & (nbins - 1))];
        ELBA_REQUIRE(std::equal(own.begin(), own.end(), counts), ELBA_ERR_INVALID_ARG, "primcheck: first histogram: the rows are not the keys' digit counts");
        a.upload(k0, (size_t)n * 8); c.upload(k1, (size_t)n * 8);
        ELBA_HIP(hipMemcpy(d_hist, counts, own.size() * 4, hipMemcpyHostToDevice));
        const void *before = tmp.p;
        *where = elba::radix_sort_keys(nullptr, a.as<uint64_t>(), c.as<uint64_t>(), n, bit_lo, bit_hi, tmp, true);
        ELBA_REQUIRE(tmp.p == before, ELBA_ERR_INTERNAL, "primcheck: the sort reallocated the workspace behind radix_first_histogram");
        finish();
        a.download(k0, "k0"); c.download(k1, "k1");
    });
}

// keys[n] -> csr[n], rowptr[M + 1] (both in and out: the caller presets them)
int primcheck_radix_sort_keys_to_csr(const uint64_t *keys, int64_t n, int idbits, int pb, int rs, int mb, int pbi, int64_t M, uint64_t *csr, uint32_t *rowptr)
{
    return guarded([&] {
        ELBA_REQUIRE(n >= 1 && M >= 1 && M < (1ll << 32) && mb >= 1 && mb <= 32 && rs >= 0 && rs + mb <= 64 && idbits >= 0 && idbits <= 32 && pb >= 0 && pb <= 30 && pbi >= 0 && pbi <= 16,
                     ELBA_ERR_INVALID_ARG, "primcheck: CSR sort: field widths");
        for (int64_t z = 0; z < n; ++z)
            ELBA_REQUIRE((int64_t)((keys[z] >> rs) & ((1ull << mb) - 1)) < M, ELBA_ERR_INVALID_ARG, "primcheck: CSR sort: a key's read is not below M");
        Dev a, c, dc, dr; DevBuf tmp;
        a.upload(keys, (size_t)n * 8); c.alloc((size_t)n * 8);
        dc.upload(csr, (size_t)n * 8); dr.upload(rowptr, (size_t)(M + 1) * 4);
        const elba::CsrFin fin{idbits, pb, rs, mb, pbi, dc.as<uint64_t>(), dr.as<uint32_t>(), M};
        elba::radix_sort_keys_to_csr(nullptr, a.as<uint64_t>(), c.as<uint64_t>(), n, fin, tmp);
        finish();
        std::vector<uint64_t> scratch((size_t)n);
        a.download(scratch.data(), "k0"); c.download(scratch.data(), "k1");
        dc.download(csr, "csr"); dr.download(rowptr, "rowptr");
    });
}

}  // extern "C"
