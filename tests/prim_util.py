"""The test-only harness over the device primitives (tests/primcheck, libelba_primcheck.so) behind ctypes, and the plain references its
results are compared with: numpy and Python integers only, nothing shared with the code under test.  Not product ABI."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRIMCHECK_DIR = os.path.join(ROOT, "tests", "primcheck")
PRIMCHECK_LIB = os.path.join(PRIMCHECK_DIR, "libelba_primcheck.so")

RS_MAXBITS = 9          # prims.hip: widest digit of the radix sort
RS_TILE = 8192          # prims.hip: keys per tile of the sort (256 x 32 keys, 1024 x 8 pairs)
SCAN_TILE = 2048        # prims.hip: items per workgroup of the scans
CS_ROWS = 128           # prims.hip: histogram rows one workgroup of the column scan folds

ENTRY_POINTS = (
    "primcheck_last_error", "primcheck_exclusive_scan_u32", "primcheck_exclusive_scan_u32_to_i64", "primcheck_fill_u32", "primcheck_fill_u64",
    "primcheck_reduce_max_u64", "primcheck_group_offsets_u32", "primcheck_group_offsets_k32", "primcheck_radix_column_scan",
    "primcheck_radix_sort_where", "primcheck_radix_sort_pairs", "primcheck_radix_sort_pairs_k32", "primcheck_radix_sort_keys",
    "primcheck_radix_first_histogram", "primcheck_radix_sort_keys_first_hist", "primcheck_radix_sort_keys_to_csr",
)

_lib = None


class PrimcheckError(RuntimeError):
    def __init__(self, status, text):
        super().__init__("primcheck status %d: %s" % (status, text))
        self.status = status


def lib():
    """Loads the harness (building it when it is missing).  The product library is loaded first, through the package, so that both share one
    HIP runtime (elba_amd.capi.load_library)."""
    global _lib
    if _lib is not None:
        return _lib
    import elba_amd
    elba_amd.load_library()
    if not os.path.exists(PRIMCHECK_LIB):
        subprocess.check_call(["make", "-C", PRIMCHECK_DIR], stdout=subprocess.DEVNULL)
    L = C.CDLL(PRIMCHECK_LIB)
    L.primcheck_last_error.restype = C.c_char_p
    vp, i64, i32, u32, u64 = C.c_void_p, C.c_int64, C.c_int, C.c_uint32, C.c_uint64
    ip = C.POINTER(C.c_int)
    sig = {
        "primcheck_exclusive_scan_u32": [vp, vp, i64, i32],
        "primcheck_exclusive_scan_u32_to_i64": [vp, vp, i64],
        "primcheck_fill_u32": [vp, i64, u32, i64],
        "primcheck_fill_u64": [vp, i64, u64, i64],
        "primcheck_reduce_max_u64": [vp, i64, C.POINTER(u64)],
        "primcheck_group_offsets_u32": [vp, i32, i64, vp, i64],
        "primcheck_group_offsets_k32": [vp, i64, vp, i64],
        "primcheck_radix_column_scan": [vp, i64, u32],
        "primcheck_radix_sort_where": [i64, i32, i32, ip],
        "primcheck_radix_sort_pairs": [vp, vp, vp, vp, i64, i32, i32, ip],
        "primcheck_radix_sort_pairs_k32": [vp, vp, vp, vp, i64, i32, i32, ip],
        "primcheck_radix_sort_keys": [vp, vp, i64, i32, i32, ip],
        "primcheck_radix_first_histogram": [i64, i32, i32, ip, ip, ip, C.POINTER(i64)],
        "primcheck_radix_sort_keys_first_hist": [vp, vp, i64, i32, i32, vp, i64, ip],
        "primcheck_radix_sort_keys_to_csr": [vp, i64, i32, i32, i32, i32, i32, i64, vp, vp],
    }
    for name, args in sig.items():
        f = getattr(L, name)
        f.argtypes = args
        f.restype = i32
    _lib = L
    return L


def _check(rc):
    if rc:
        raise PrimcheckError(rc, lib().primcheck_last_error().decode())


def _arr(a, dtype):
    a = np.array(a, dtype=dtype, copy=True, order="C").reshape(-1)
    return a


def _p(a):
    return a.ctypes.data if a.size else None


# ---- the harness's entries: every one copies its inputs, so the caller's arrays are never changed ------------------------------------
def scan_u32(x, inplace=False, preset=0xDEADBEEF):
    x = _arr(x, np.uint32)
    out = np.full(x.size, preset, dtype=np.uint32)
    _check(lib().primcheck_exclusive_scan_u32(_p(x), _p(out), x.size, 1 if inplace else 0))
    return out


def scan_u32_to_i64(x, preset=-7):
    x = _arr(x, np.uint32)
    out = np.full(x.size, preset, dtype=np.int64)
    _check(lib().primcheck_exclusive_scan_u32_to_i64(_p(x), _p(out), x.size))
    return out


def fill(dtype, total, v, n, preset):
    buf = np.full(total, preset, dtype=dtype)
    f = lib().primcheck_fill_u32 if np.dtype(dtype) == np.uint32 else lib().primcheck_fill_u64
    _check(f(_p(buf), total, v, n))
    return buf


def reduce_max(x):
    x = _arr(x, np.uint64)
    out = C.c_uint64(12345)
    _check(lib().primcheck_reduce_max_u64(_p(x), x.size, C.byref(out)))
    return int(out.value)


def group_offsets(keys, nkeys, key_shift=0, k32=False, preset=0xDEADBEEF):
    keys = _arr(keys, np.uint32 if k32 else np.uint64)
    ptr = np.full(nkeys + 1, preset, dtype=np.uint32)
    if k32:
        _check(lib().primcheck_group_offsets_k32(_p(keys), keys.size, _p(ptr), nkeys))
    else:
        _check(lib().primcheck_group_offsets_u32(_p(keys), key_shift, keys.size, _p(ptr), nkeys))
    return ptr


def column_scan(rows):
    rows = np.array(rows, dtype=np.uint32, copy=True, order="C")
    nrows, nbins = rows.shape
    _check(lib().primcheck_radix_column_scan(rows.ctypes.data, nrows, nbins))
    return rows


def sort_where(n, lo, hi):
    w = C.c_int(-1)
    _check(lib().primcheck_radix_sort_where(n, lo, hi, C.byref(w)))
    return int(w.value)


OTHER_KEY = 0x0123456789ABCDEF      # what the second buffer pair holds before a sort: recognisable when it is left alone
OTHER_VAL = 0xFEDCBA9876543210


def sort_pairs(keys, vals, lo, hi, k32=False):
    """-> (where, (k0, v0), (k1, v1)): both buffer pairs after the call"""
    kt = np.uint32 if k32 else np.uint64
    k0, v0 = _arr(keys, kt), _arr(vals, np.uint64)
    k1 = np.full(k0.size, OTHER_KEY & (0xFFFFFFFF if k32 else 0xFFFFFFFFFFFFFFFF), dtype=kt)
    v1 = np.full(k0.size, OTHER_VAL, dtype=np.uint64)
    w = C.c_int(-1)
    f = lib().primcheck_radix_sort_pairs_k32 if k32 else lib().primcheck_radix_sort_pairs
    _check(f(_p(k0), _p(v0), _p(k1), _p(v1), k0.size, lo, hi, C.byref(w)))
    return int(w.value), (k0, v0), (k1, v1)


def sort_keys(keys, lo, hi):
    """-> (where, k0, k1)"""
    k0 = _arr(keys, np.uint64)
    k1 = np.full(k0.size, OTHER_KEY, dtype=np.uint64)
    w = C.c_int(-1)
    _check(lib().primcheck_radix_sort_keys(_p(k0), _p(k1), k0.size, lo, hi, C.byref(w)))
    return int(w.value), k0, k1


def first_histogram_layout(n, lo, hi):
    """-> (shift, bits, tile, byte offset of the rows in the workspace)"""
    s, b, t, o = C.c_int(-1), C.c_int(-1), C.c_int(-1), C.c_int64(-1)
    _check(lib().primcheck_radix_first_histogram(n, lo, hi, C.byref(s), C.byref(b), C.byref(t), C.byref(o)))
    return int(s.value), int(b.value), int(t.value), int(o.value)


def sort_keys_first_hist(keys, lo, hi, counts):
    k0 = _arr(keys, np.uint64)
    k1 = np.full(k0.size, OTHER_KEY, dtype=np.uint64)
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    w = C.c_int(-1)
    _check(lib().primcheck_radix_sort_keys_first_hist(_p(k0), _p(k1), k0.size, lo, hi, counts.ctypes.data, counts.shape[0], C.byref(w)))
    return int(w.value), k0, k1


def sort_keys_to_csr(words, fin, M, preset_csr=0x5555555555555555, preset_rowptr=0x77777777):
    """fin = dict(idbits, pb, rs, mb, pbi) -> (csr[n], rowptr[M + 1])"""
    words = _arr(words, np.uint64)
    csr = np.full(words.size, preset_csr, dtype=np.uint64)
    rowptr = np.full(M + 1, preset_rowptr, dtype=np.uint32)
    _check(lib().primcheck_radix_sort_keys_to_csr(_p(words), words.size, fin["idbits"], fin["pb"], fin["rs"], fin["mb"], fin["pbi"], M, _p(csr), _p(rowptr)))
    return csr, rowptr


# ---- references ------------------------------------------------------------------------------------------------------------------------
def radix_digits(lo, hi):
    """prims.hip's radix_digits restated: [(shift, bits)] of the passes of a sort of the bits [lo, hi) — as even as they come, at most
    RS_MAXBITS wide, the remainder spread over the first passes"""
    B = hi - lo
    npass = (B + RS_MAXBITS - 1) // RS_MAXBITS
    out, at = [], lo
    for q in range(npass):
        bits = B // npass + (1 if q < B % npass else 0)
        out.append((at, bits))
        at += bits
    return out


def sort_where_ref(n, lo, hi):
    return 0 if (n <= 1 or hi <= lo) else len(radix_digits(lo, hi)) & 1


def sort_field(keys, lo, hi):
    """the bits [lo, hi) of every key, as uint64"""
    keys = np.asarray(keys).astype(np.uint64)
    width = hi - lo
    mask = np.uint64((1 << width) - 1)
    return (keys >> np.uint64(lo)) & mask


def stable_order(keys, lo, hi):
    """the permutation a stable sort on the bits [lo, hi) applies"""
    return np.argsort(sort_field(keys, lo, hi), kind="stable")


def exclusive_scan_exact(x):
    """exclusive prefix sums of uint32 values as exact uint64 (sums stay far below 2^64: n * 2^32)"""
    x = np.asarray(x, dtype=np.uint64)
    out = np.zeros(x.size, dtype=np.uint64)
    if x.size > 1:
        np.cumsum(x[:-1], out=out[1:])
    return out


def group_offsets_ref(keys, nkeys, key_shift=0):
    """ptr[k] = first index z with (keys[z] >> key_shift) >= k, k in [0, nkeys]"""
    g = np.asarray(keys).astype(np.uint64) >> np.uint64(key_shift)
    return np.searchsorted(g, np.arange(nkeys + 1, dtype=np.uint64), side="left").astype(np.uint32)


def column_scan_ref(rows):
    """rows[t][d] -> the place of tile t's first key with digit d: the counts of all smaller digits in every tile + the counts of d in
    the tiles before t (the total must stay below 2^32)"""
    r = np.asarray(rows, dtype=np.uint64)
    tot = r.sum(axis=0)
    base = np.zeros(r.shape[1], dtype=np.uint64)
    base[1:] = np.cumsum(tot)[:-1]
    down = np.zeros_like(r)
    if r.shape[0] > 1:
        np.cumsum(r[:-1], axis=0, out=down[1:])
    out = down + base[None, :]
    assert int(tot.sum()) < 1 << 32
    return out.astype(np.uint32)


def csr_plain_word(read, kid, hint, pos, fin):
    """a plain sort key of the CSR build (matrix.hip: k_csc_to_csr_words): read << rs | id << (pb + 2) | hint << pb | pos"""
    return (int(read) << fin["rs"]) | (int(kid) << (fin["pb"] + 2)) | (int(hint) << fin["pb"]) | int(pos)


def csr_inline_word(read, partner, pos_q, pos_t, fin):
    """an inline-partner key: bit 63 | read << rs | (partner >> 1) << 2 pbi | posQ << pbi | posT"""
    return (1 << 63) | (int(read) << fin["rs"]) | ((int(partner) >> 1) << (2 * fin["pbi"])) | (int(pos_q) << fin["pbi"]) | int(pos_t)


def csr_unpack_ref(words, fin, M):
    """matrix.hip's k_unpack_csr_words restated on the words sorted stably by their read: -> (csr[n], rowptr[M + 1])"""
    words = np.asarray(words, dtype=np.uint64)
    rs, mb, pb, pbi, idbits = fin["rs"], fin["mb"], fin["pb"], fin["pbi"], fin["idbits"]
    w = words[stable_order(words, rs, rs + mb)]
    reads = sort_field(w, rs, rs + mb)
    u = np.uint64
    inline = (w >> u(63)) != 0
    pm = u((1 << pbi) - 1)
    e_inl = (u(1) << u(63)) | (((w >> u(2 * pbi)) & u((1 << (mb - 1)) - 1)) << u(32)) | ((w >> u(pbi)) & pm) | ((w & pm) << u(16))
    e_pln = (((w >> u(pb + 2)) & u((1 << idbits) - 1)) << u(32)) | (((w >> u(pb)) & u(3)) << u(30)) | (w & u((1 << pb) - 1))
    csr = np.where(inline, e_inl, e_pln)
    rowptr = np.searchsorted(reads, np.arange(M + 1, dtype=np.uint64), side="left").astype(np.uint32)
    return csr, rowptr


# ---- the FASTA encoder's boundary grid (tests/test_gpu_ingest.py on the device, tests/test_prim_reference_cpu.py for its arithmetic) ------
# ingest.hip encodes a read in trips of 4096 bases: lengths around one, two and three trips, a long read, the shortest ones and an empty record
INGEST_LENGTHS = (4095, 4096, 4097, 8191, 8192, 8193, 12289, 70001, 1, 2, 3, 4, 5, 0)
INGEST_WIDTHS = (1, 7, 60, 61, 80, 4095, 4096, 4097, 0)      # bases per line; 0 = the whole read on one line
INGEST_ALPHABET = b"ACGTacgtNnXR"      # incl. characters outside the code table


def ingest_grid_seqs(seed, lengths=INGEST_LENGTHS):
    rng = np.random.default_rng(seed)
    alphabet = np.frombuffer(INGEST_ALPHABET, dtype=np.uint8)
    return [alphabet[rng.integers(0, len(alphabet) if i % 3 == 0 else 8, n)].tobytes() for i, n in enumerate(lengths)]


def write_fasta(path, seqs, width, final_newline=True, place=None):
    """One record per read, lines of `width` bases (<= 0: one line); an empty read is a header followed by an empty line.
    place = (i, m): the header of record i is padded so that the record's first base lies at a file offset that is m modulo 16."""
    out = bytearray()
    for i, s in enumerate(seqs):
        head = b">read%d some description" % i
        if place is not None and i == place[0]:
            head += b"x" * ((place[1] - (len(out) + len(head) + 1)) % 16)
        out += head + b"\n"
        if width <= 0 or not s:
            out += s + b"\n"
        else:
            for a in range(0, len(s), width):
                out += s[a:a + width] + b"\n"
    if not final_newline:
        assert out.endswith(b"\n")
        del out[-1]
    with open(path, "wb") as f:
        f.write(bytes(out))
