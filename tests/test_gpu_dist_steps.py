"""-m gpu: the device calls of the sharded build of A (elba_dist_* of include/elba_amd.h), ONE call at a time, against the scripted worlds of
tests/dist_step_cases.py.  A HipBackend context plays one rank of a world of up to 64 while the script (dist_sim.NumpyBackend on the oracle's
enumerator) plays all the others: every other rank's messages are the script's, every output of the device rank is compared with the script's
at once, exact integer equality, the step's name in the message.  No threads, no ThreadedGroup; one context at a time, closed before the next.

Steps per rank (dist_step_cases.replay): value_histogram; count_owners + fill_send; packed_format (+ fill_send_packed; unpack_records whole
and in two rounds through out= slices); count_records, the reliable k-mers by copy and by pointer (and the ABI's answers for k > 31 and for a
short buffer); global ids by base AND by the gathered union on the same context, panel_counts + panel_fill after each; the windowed panel
calls for every window set of the case; set_panel + create_seed_matrix + export_csr of the script's incoming panel.

What each case pins is stated, and checked on the CPU, in tests/test_dist_steps_cpu.py.

Wall time per test on one MI355X (s), all device ranks of the case, the case's script built in the same call; 17 tests in 5.9 s:
    short_reads 0.51 (the first to load the library)   empty_ranks 0.08   owners_64_hist 0.30   owners_64_hand 0.31
    packed_k27_fits 0.03   packed_k27_over 0.03   packed_k31_fits 0.14   packed_k31_over 0.10   packed_k7 0.03   packed_k5 0.01
    multiword_33 0.11   multiword_65 0.09   count_edges 2,4: 0.04   3,3: 0.04   2,40: 0.08   panel_windows_64 1.19   panel_windows_3 0.73

That the comparisons bite, on scratch builds of kmer.hip with one comparison changed each (never committed):
    owner_of `<=` for `<`                  owner_counts differs: short_reads, empty_ranks, both owners_64, packed_k27 / k31, multiword_33, panel_windows
    k_dist_unpack's search `<` for `<=`    unpack differs: every case with 8-byte records (short_reads rank 0 at record 0, empty_ranks, owners_64, ...)
    k_panel's window `<=` for `<` above    panel_counts_win1 (win_lo == win_hi for the odd ranks) differs: panel_windows_64 and panel_windows_3
"""
import ctypes as C

import numpy as np
import pytest

import dist_step_cases as dsc
from elba_amd import capi
from elba_amd.distributed import HipBackend, kmer_words

pytestmark = pytest.mark.gpu

ELBA_ERR_INVALID_ARG, ELBA_ERR_UNSUPPORTED = 1, 6


def _reliable_kmer_abi(be, sc, r, rel):
    """elba_dist_get_reliable_kmers (k <= 31: the same n and words; k > 31: ELBA_ERR_UNSUPPORTED) and elba_dist_copy_reliable_kmers with a
    buffer one k-mer short (ELBA_ERR_INVALID_ARG), right after the copy that produced `rel`"""
    k, n, kw = sc.case.k, len(rel), kmer_words(sc.case.k)
    where = "%s, rank %d: " % (sc.case.name, r)
    ptr, cnt = C.c_void_p(), C.c_int64(-1)
    rc = be.L.elba_dist_get_reliable_kmers(be.h, C.byref(ptr), C.byref(cnt))
    if k <= 31:
        assert rc == 0 and cnt.value == n, where + "get_reliable_kmers: status %d, n %d, want %d" % (rc, cnt.value, n)
        got = capi._copy_from_device(ptr.value, n, np.uint64)
        assert np.array_equal(got, rel.reshape(-1)), where + "get_reliable_kmers: the words differ from copy_reliable_kmers'"
    else:
        assert rc == ELBA_ERR_UNSUPPORTED, where + "get_reliable_kmers at k > 31: status %d" % rc
    if n > 0:
        small = be.empty_words((n - 1) * kw + 1)
        rc = be.L.elba_dist_copy_reliable_kmers(be.h, small.data_ptr(), n - 1)
        assert rc == ELBA_ERR_INVALID_ARG, where + "copy_reliable_kmers with capacity own_N - 1: status %d" % rc


def _play(name, ranks=None, record_order=None):
    """the case's device ranks, one context each, every step checked against the script as soon as it is there"""
    sc = dsc.script(name)
    c = sc.case
    for r in (c.device_ranks if ranks is None else ranks):
        be = HipBackend(c.k, c.lower, c.upper, 0)
        try:
            against = dsc.checker(sc, r)

            def check(step, got):
                against(step, got)
                if step == "rel":
                    _reliable_kmer_abi(be, sc, r, got)

            order = None if record_order is None else dsc.record_orders(len(sc.recv16[r]))[record_order]
            out = dsc.replay(be, sc, r, check=check, record_order=order)
            assert set(out) == set(sc.steps) - {"gid"}, (name, r)
        finally:
            be.e.close()
    return sc


def test_short_reads():
    """reads of 1, k - 1, k, k + 1 bases at the start, in the middle (at a wavefront's first instance and inside a wavefront) and at the end of a shard"""
    _play("short_reads")


def test_empty_ranks():
    """ranks without reads and a rank whose reads are all shorter than k: they own k-mers all the same; senders with zero reads in unpack_records"""
    _play("empty_ranks")


@pytest.mark.parametrize("name", ["owners_64_hist", "owners_64_hand"])
def test_owners_64(name):
    """64 owners: every LDS counter of the senders in use; by hand, owners 0, 31 and 63 have empty ranges (repeated boundaries)"""
    _play(name)


@pytest.mark.parametrize("name", ["packed_k27_fits", "packed_k27_over", "packed_k31_fits", "packed_k31_over", "packed_k7", "packed_k5"])
def test_packed_limit(name):
    """value bits + index bits at 64 and at 65 (k = 27 with two owners, k = 31 with 64), one owner at k = 7, never at k = 5"""
    sc = _play(name)
    assert (sc.fmt is None) == (name in ("packed_k27_over", "packed_k31_over", "packed_k5"))


@pytest.mark.parametrize("k", [33, 65])
def test_multiword(k):
    """24- and 32-byte records, the owner's multi-word sort, interleaved reliable k-mers, set_global_kmers with two and three words"""
    _play("multiword_%d" % k)


@pytest.mark.parametrize("lower,upper", [(2, 4), (3, 3), (2, 40)])
def test_count_edges(lower, upper):
    """counts LOWER - 1 .. UPPER + 1 on one owner, a read that holds a reliable k-mer twice, columns of up to 40 entries — with the records as
    sent, reversed (the column sort's worst case) and shuffled: statistics, reliable k-mers and columns (the panel records) are the script's each time"""
    name = "count_edges_%d_%d" % (lower, upper)
    _play(name, ranks=(0, 1))
    _play(name, ranks=(0, 1), record_order="reversed")
    _play(name, ranks=(0,), record_order="shuffled")


@pytest.mark.parametrize("W", [64, 3])
def test_panel_windows(W):
    """a column with reads of the first and the last rank only, an owner without a reliable k-mer, own_N no multiple of 64; row blocks: whole
    ranks, empty ones, one row at a rank's first and last row, a block that no column reaches"""
    _play("panel_windows_%d" % W)
