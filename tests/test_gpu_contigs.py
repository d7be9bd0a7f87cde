"""-m gpu: contig generation on the GPU (elba_generate_contigs, contig.hip) against the restatement of GenerateContigs in contig_util.py,
fed with the GPU's own exported S and, end to end, with the oracle's S.  Every byte of every contig, the chains, the read map, the counts."""
import ctypes as C

import numpy as np
import pytest

import contig_util as cu
import elba_amd
import gpu_util as gu
import hostcpp_util as hu
from elba_amd import formats
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

STATS = ("nreads", "branches", "components", "used_components", "contigs", "cycles", "contig_reads", "bases", "longest")


def _check(e, st, seqs, S=None):
    """The GPU's contigs, chains, read map and counts equal the restatement's on S (default: the GPU's own exported S)."""
    M = len(seqs)
    if S is None:
        g = e.export_string_graph()
        S = (g["rows"], g["cols"], g["vals"])
    contigs, chains, read_contig, xst = cu.generate_contigs(M, *S, seqs)
    for k in STATS:
        assert st[k] == xst[k], (k, st, xst)
    got = e.export_contigs()
    assert got["n"] == len(contigs)
    assert got["seqs"] == contigs
    co = got["chain_off"]
    assert len(co) == len(contigs) + 1 and co[0] == 0
    for i, ch in enumerate(chains):
        a, b = int(co[i]), int(co[i + 1])
        assert list(zip(got["chain_read"][a:b].tolist(), got["chain_prefix"][a:b].tolist(), got["chain_strand"][a:b].tolist())) == ch, i
    assert (e.export_read_contigs(M) == np.array(read_contig, dtype=np.int64)).all()
    assert st["ms_total"] > 0 and st["ms_rank"] >= 0
    return contigs


def _engine_with(packed, off, lens, rows, cols, vals, fuzz=1000):
    e = elba_amd.Engine(17, 2, 8)
    e.set_reads(packed, off, lens)
    e.set_overlaps(len(lens), rows, cols, vals)
    s = e.transitive_reduction(0.0, fuzz)
    return e, s


@pytest.mark.parametrize("seed", range(8))
def test_random_string_graphs(seed):
    rng = np.random.default_rng(700 + seed)
    M = int(rng.integers(40, 3000))
    seqs = cu.random_reads(rng, M, 1 if seed % 2 else 20, 300)
    packed, off, lens = cu.pack(seqs)
    rows, cols, vals = cu.random_string_graph(rng, M, lens, n_paths=int(rng.integers(1, M // 4 + 2)), p_extra=float(rng.choice([0.0, 0.05, 0.3])))
    e, s = _engine_with(packed, off, lens, rows, cols, vals)
    assert s["nnz"] == 2 * len(rows)                         # no triangles: S is the input, both triangles
    st = e.generate_contigs()
    contigs = _check(e, st, seqs)
    assert st["contigs"] > 0 and st["bases"] == sum(len(c) for c in contigs)
    e.close()


def _planted(rng, M, parts):
    """Paths / cycles of the given sizes on shuffled ids; suffix and suffixT in [5, 9] so that no entry is transitive at fuzz 0 (a two-edge
    path is at least 10 > 9): S equals the input even where the parts form triangles (3-cycles)."""
    perm = rng.permutation(M)
    edges, at = {}, 0
    for size, cyc in parts:
        seg = perm[at:at + size]; at += size
        pairs = list(zip(seg[:-1], seg[1:])) + ([(seg[-1], seg[0])] if cyc else [])
        for x, y in pairs:
            i, j = int(min(x, y)), int(max(x, y))
            o = cu.edge(rng, 20, 20)
            o["suffix"] = int(rng.integers(5, 10)); o["suffixT"] = int(rng.integers(5, 10))
            edges[(i, j)] = o
    assert at <= M
    return cu.upper(edges)


@pytest.mark.parametrize("case", ["one_long_path", "mixed_paths", "cycles"])
def test_long_paths_and_cycles(case):
    rng = np.random.default_rng({"one_long_path": 1, "mixed_paths": 2, "cycles": 3}[case])
    if case == "one_long_path":
        parts = [(200000, False)]
    elif case == "mixed_paths":
        sizes = [1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 31, 33, 64, 65, 127, 129, 255, 257, 1000, 1023, 1025, 2047, 2049, 4095, 4097, 5000]
        sizes += rng.integers(1, 5001, 40).tolist()
        parts = [(int(s), False) for s in sizes]
    else:
        sizes = [3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 33, 100, 1000, 1024, 1025, 4096, 10000] + rng.integers(3, 200, 30).tolist()
        parts = [(int(s), True) for s in sizes] + [(50, False), (2, False)]
    M = sum(p[0] for p in parts) + 5                         # + 5 isolated reads
    packed, off, lens = cu.random_packed(rng, M, 20, 40)
    seqs = cu.seqs_of(packed, off, lens)
    rows, cols, vals = _planted(rng, M, parts)
    e, s = _engine_with(packed, off, lens, rows, cols, vals, fuzz=0)
    assert s["nnz"] == 2 * len(rows)
    st = e.generate_contigs()
    _check(e, st, seqs)
    assert st["cycles"] == sum(1 for size, cyc in parts if cyc)
    assert st["contigs"] == sum(1 for size, cyc in parts if not cyc and size >= 2)
    assert st["branches"] == 0
    if case == "one_long_path":
        assert st["contig_reads"] == 200000
    e.close()


@pytest.mark.parametrize("err", [0.0, 0.02, 0.10])
def test_end_to_end_against_the_oracle(err):
    """reads -> B -> x-drop alignments -> string graph -> contigs on one context, against the restatement fed with the GPU's S and with
    the oracle's S (the inputs of test_string_graph_of_aligned_reads)."""
    packed, off, lens, info = elba_amd.synth_reads(41, 120000, 14, 3000, 600, error_rate=err, min_len=400)
    seqs = cu.seqs_of(packed, off, lens)
    e, ks, ms, st = gu.gpu_full(packed, off, lens, 17, 2, 12)
    e.align_seeds()
    e.transitive_reduction(0.65, 1000)
    cst = e.generate_contigs()
    contigs = _check(e, cst, seqs)
    o = gu.oracle_run(packed, off, lens, 17, 2, 12)
    rows, cols, ov, _ = o.align_upper(packed, off, lens, nthreads=8)
    S, _, _ = po.string_graph(len(lens), rows, cols, ov, cutoff=0.65, fuzz=1000)
    assert _check(e, cst, seqs, (S["rows"], S["cols"], S["vals"])) == contigs
    if err <= 0.02:                                          # (at 10 % error the bad-read prune leaves S without paths on this set)
        assert cst["contigs"] > 0
    e.close()


def test_error_free_contigs_are_genome_substrings():
    """At error 0 without repeats every contig is a substring of the genome or of its reverse complement."""
    packed, off, lens, info = elba_amd.synth_reads(43, 80000, 12, 3000, 600, error_rate=0.0, min_len=400)
    seqs = cu.seqs_of(packed, off, lens)
    glen = int(max(info["genome_pos"][i] + lens[i] for i in range(len(lens))))
    g = ["N"] * glen
    for i, s in enumerate(seqs):
        p = int(info["genome_pos"][i])
        fwd = cu.revcomp(s) if info["strand"][i] else s
        g[p:p + len(fwd)] = fwd
    G = "".join(g)
    Grc = cu.revcomp(G)
    e, _, _, _ = gu.gpu_full(packed, off, lens, 17, 2, 12)
    e.align_seeds()
    e.transitive_reduction(0.65, 1000)
    st = e.generate_contigs()
    contigs = _check(e, st, seqs)
    assert st["contigs"] > 0
    bad = [i for i, c in enumerate(contigs) if c not in G and c not in Grc]
    assert not bad, (len(bad), len(contigs))
    e.close()


def test_errors_and_invalidation():
    rng = np.random.default_rng(11)
    seqs = cu.random_reads(rng, 60)
    packed, off, lens = cu.pack(seqs)
    rows, cols, vals = _planted(rng, 60, [(20, False), (15, False), (10, False)])      # every edge on a path: every entry is walked
    e = elba_amd.Engine(17, 2, 8)
    with pytest.raises(elba_amd.ElbaError) as x:                 # no S
        e.generate_contigs()
    assert x.value.status == 5
    e.set_overlaps(60, rows, cols, vals)
    e.transitive_reduction(0.0, 1000)
    with pytest.raises(elba_amd.ElbaError) as x:                 # S, but the reads are not on the context
        e.generate_contigs()
    assert x.value.status == 5
    e.set_reads(packed, off, lens)                               # set_reads then set_overlaps keeps both
    e.set_overlaps(60, rows, cols, vals)
    e.transitive_reduction(0.0, 1000)
    st = e.generate_contigs()
    first = _check(e, st, seqs)
    st2 = e.generate_contigs()                                   # a second call gives the same output
    assert all(st[k] == st2[k] for k in STATS) and e.export_contigs()["seqs"] == first
    e.transitive_reduction(0.0, 1000)                            # a new S invalidates the contigs
    with pytest.raises(elba_amd.ElbaError) as x:
        e.export_contigs()
    assert x.value.status == 5
    with pytest.raises(elba_amd.ElbaError):
        e.export_read_contigs(60)
    # a suffixT outside [0, len]: the call fails naming the pair, nothing is exported
    bad = vals.copy()
    bad["suffixT"][0] = int(lens[rows[0]]) + 1
    bad["suffix"][0] = -3
    e.set_overlaps(60, rows, cols, bad)
    e.transitive_reduction(0.0, 1000)
    g = e.export_string_graph()
    with pytest.raises(cu.BadPrefix):
        cu.generate_contigs(60, g["rows"], g["cols"], g["vals"], seqs)
    with pytest.raises(elba_amd.ElbaError) as x:
        e.generate_contigs()
    assert x.value.status == 1 and "prefix" in str(x.value)
    with pytest.raises(elba_amd.ElbaError):
        e.export_contigs()
    # an empty S: no contigs
    e.set_overlaps(60, rows[:0], cols[:0], vals[:0])
    e.transitive_reduction(0.0, 1000)
    st = e.generate_contigs()
    assert st["contigs"] == 0 and st["components"] == 60 and e.export_contigs()["seqs"] == []
    assert (e.export_read_contigs(60) == -1).all()
    e.close()


def test_replicated_reads_serve_the_graph():
    """A context whose own reads are not the graph's takes them from elba_dist_set_all_reads."""
    import torch
    rng = np.random.default_rng(12)
    seqs = cu.random_reads(rng, 80)
    packed, off, lens = cu.pack(seqs)
    rows, cols, vals = cu.random_string_graph(rng, 80, lens, n_paths=8, p_extra=0.1)
    e = elba_amd.Engine(17, 2, 8)
    e.set_reads(*cu.pack(seqs[:10]))                             # a shard of the reads
    dp = torch.from_numpy(packed.astype(np.uint8)).cuda(); do = torch.from_numpy(off.astype(np.int64)).cuda(); dl = torch.from_numpy(lens.astype(np.int32)).cuda()
    torch.cuda.synchronize()
    L = e.L                                                      # (the prototype elba_amd/distributed.py declares)
    L.elba_dist_set_all_reads.restype = C.c_int
    L.elba_dist_set_all_reads.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64]
    e._check(L.elba_dist_set_all_reads(e.h, dp.data_ptr(), len(packed) - 16, do.data_ptr(), dl.data_ptr(), 80))
    e.set_overlaps(80, rows, cols, vals)
    e.transitive_reduction(0.0, 1000)
    _check(e, e.generate_contigs(), seqs)
    e.close()


def test_host_mirror_writes_the_same_contigs_fa(tmp_path):
    packed, off, lens, info = elba_amd.synth_reads(44, 60000, 12, 3000, 500, error_rate=0.01, min_len=400)
    seqs = cu.seqs_of(packed, off, lens)
    fa = hu.write_fasta(tmp_path / "reads.fa", seqs)
    out = tmp_path / "cpp.contigs.fa"
    hu.run_json(hu.binary("test_host_contigs"), [fa, 17, 2, 12, out])
    e, _, _, _ = gu.gpu_full(packed, off, lens, 17, 2, 12)
    e.align_seeds()
    e.transitive_reduction(0.65, 1000)
    e.generate_contigs()
    got = e.export_contigs()
    ref = tmp_path / "py.contigs.fa"
    formats.write_contigs_fasta(str(ref), got["seqs"])
    assert got["n"] > 0 and out.read_bytes() == ref.read_bytes()
    e.close()
