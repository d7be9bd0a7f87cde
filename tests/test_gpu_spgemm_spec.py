"""The reads-path instantiation of the SpGEMM's numeric kernel (k_spgemm_direct<..., SPEC = true>, spgemm.hip: ov_spec_ok).

Reads built like the headline workload's (15 %-error long reads, k = 17, L = 2, U = 8: padded columns with inline partners, 32-bit accumulators
carrying posT, 16-byte records) must take it (stat "overlap_spec" = 1) and give the oracle's B; the general kernel, forced through option
"ov_generic" on the same engine, must give the same B bit for bit and the same statistics; every knob that changes one of the switches the
instantiation fixes must take the general kernel and still give the oracle's B."""
import numpy as np
import pytest

import elba_amd
import gpu_util as gu

pytestmark = pytest.mark.gpu

# (seed, genome, depth, avg_len, sd_len, error, min_len): the headline's read model on a smaller genome.  "small": ~2000 rows — no sampled rows
# and no mirror slabs on a cold call; "sampled": >= 8192 rows — a cold call computes a sample of rows first and the mirror slabs are on.
SHAPES = {
    "small": (7, 200_000, 30.0, 3000.0, 500.0, 0.15, 1000),
    "sampled": (8, 900_000, 30.0, 3000.0, 500.0, 0.15, 1000),
}
# (rows forwarded / escalated to a larger tier are left out: on a call without a measured ratio they depend on which rows finish first)
STATS = ("overlap_spec", "overlap_slab_q16", "overlap_mirror_placed")

_cache = {}


def _shape(name):
    if name not in _cache:
        seed, genome, depth, avg, sd, err, mn = SHAPES[name]
        packed, off, lens, info = elba_amd.synth_reads(seed, genome, depth, avg, sd, error_rate=err, min_len=mn)
        _cache[name] = (packed, off, lens, gu.oracle_run(packed, off, lens, 17, 2, 8))
    return _cache[name]


def _same_B(a, b):
    assert a["Y"] == b["Y"]
    assert (a["rowptr"] == b["rowptr"]).all() and (a["col"] == b["col"]).all()
    assert np.array_equal(a["val"], b["val"])


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_reads_built_matrices_take_the_reads_path_kernel(shape):
    packed, off, lens, o = _shape(shape)
    if shape == "sampled":
        assert len(lens) >= 8192
    e, ks, ms, st = gu.gpu_full(packed, off, lens, 17, 2, 8)
    assert e.get_stat("overlap_spec") == 1
    gu.assert_B_equal(e.export_csr(), o.B())
    gu.assert_stats_equal(st, o)
    # cold calls on the same engine: the reads-path kernel, then the general one (option "ov_generic"): the same B, bit for bit, and the same statistics
    e.set_option("overlap_cold_calls", 1)
    st_s = e.create_seed_matrix()
    B_s = e.export_csr()
    stats_s = {n: e.get_stat(n) for n in STATS}
    e.set_option("ov_generic", 1)
    st_g = e.create_seed_matrix()
    B_g = e.export_csr()
    stats_g = {n: e.get_stat(n) for n in STATS}
    assert stats_s["overlap_spec"] == 1 and stats_g["overlap_spec"] == 0
    _same_B(B_s, B_g)
    gu.assert_B_equal(B_g, o.B())
    for key in ("nnz", "products", "nnz_before_prune", "nnz_diag", "nnz_upper", "max_numshared"):
        assert st_s[key] == st_g[key], key
    for n in STATS[1:]:
        assert stats_s[n] == stats_g[n], n
    if shape == "sampled":
        assert stats_s["overlap_slab_q16"] > 0
    # and back: a steady call after the general one takes the reads-path kernel again
    e.set_option("ov_generic", 0)
    e.set_option("overlap_cold_calls", 0)
    e.create_seed_matrix()
    assert e.get_stat("overlap_spec") == 1
    _same_B(e.export_csr(), B_s)
    e.close()


@pytest.mark.parametrize("knob", [("no_symmetry", 1), ("no_ell", 1), ("no_pay", 1), ("mir32", 1), ("no_hints", 1), ("tune3", 1), ("dk", 1)])
def test_knobs_that_change_the_switches_take_the_general_kernel(knob):
    packed, off, lens, o = _shape("small")
    e, ks, ms, st = gu.gpu_full(packed, off, lens, 17, 2, 8, options={knob[0]: knob[1]})
    assert e.get_stat("overlap_spec") == 0
    gu.assert_B_equal(e.export_csr(), o.B())
    gu.assert_stats_equal(st, o)
    e.close()
