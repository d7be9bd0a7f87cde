"""The induced sub-problem of one part (elba_induce_part, include/elba_amd.h) restated on the CPU, numpy only: the rule twice (a literal
loop over reads and pairs; a vectorised form on whole arrays), the bad-read rule with outside counts, hand cases with their claims, a
builder of multi-component inputs (several string_graph_util graphs on disjoint id ranges, ids interleaved, failed pairs planted between
components, one read planted whose bad flag depends on the pairs that leave its part), and the driver that assembles an input part by
part on a second Engine and maps every result back through old_of_new."""
import numpy as np

import string_graph_util as sg
from oracle import pyoracle as po

FIELDS = tuple(f for f in po.OVERLAP_DTYPE.names if f != "pad")


# ---- the rule, twice -----------------------------------------------------------------------------------------------------------------
def _packed_bytes(lens):
    return (np.asarray(lens, dtype=np.int64) + 3) // 4


def induce_loop(M, rows, cols, vals, part_of_read, part, reads=None):
    """The rule by a literal loop.  reads = (packed, byte_off, lens) or None.  Returns the dict elba_induce_part's binding returns (host
    arrays only) plus split_pairs / split_passed."""
    old_of_new, new_of_old = [], {}
    for v in range(int(M)):
        if int(part_of_read[v]) == int(part):
            new_of_old[v] = len(old_of_new)
            old_of_new.append(v)
    R = len(old_of_new)
    oa, op = [0] * R, [0] * R
    kr, kc, kv = [], [], []
    split = split_passed = 0
    for a in range(len(rows)):
        r, c = int(rows[a]), int(cols[a])
        sr, sc = r in new_of_old, c in new_of_old
        if sr and sc:
            kr.append(new_of_old[r]); kc.append(new_of_old[c]); kv.append(a)
        elif sr != sc:
            w = new_of_old[r if sr else c]
            oa[w] += 1; split += 1
            if vals[a]["passed"] != 0:
                op[w] += 1; split_passed += 1
    out = dict(reads=R, pairs=len(kr), old_of_new=np.array(old_of_new, dtype=np.int64), rows=np.array(kr, dtype=np.int64), cols=np.array(kc, dtype=np.int64),
               vals=vals[np.array(kv, dtype=np.int64)] if kv else np.zeros(0, dtype=po.OVERLAP_DTYPE), outside_aligned=np.array(oa, dtype=np.uint32),
               outside_passed=np.array(op, dtype=np.uint32), split_pairs=split, split_passed=split_passed, packed_bytes=0)
    if reads is not None:
        packed, off, lens = reads
        buf, noff, nlen = bytearray(), [], []
        for v in old_of_new:
            L, o = int(lens[v]), int(off[v])
            b = bytearray(np.asarray(packed[o:o + (L + 3) // 4], dtype=np.uint8).tobytes())
            if L % 4:
                b[-1] &= (0xFF << (2 * (4 - L % 4))) & 0xFF      # the unused low bits of the last byte
            noff.append(len(buf)); nlen.append(L)
            buf += b
        out.update(packed_bytes=len(buf), packed=np.frombuffer(bytes(buf) + bytes(16), dtype=np.uint8).copy(), byte_off=np.array(noff, dtype=np.uint64),
                   len=np.array(nlen, dtype=np.uint32))
    return out


def induce_numpy(M, rows, cols, vals, part_of_read, part, reads=None):
    """The same on whole arrays."""
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    sel = np.asarray(part_of_read)[:int(M)] == int(part)
    old_of_new = np.flatnonzero(sel).astype(np.int64)
    new_of_old = np.cumsum(sel) - 1
    R = len(old_of_new)
    sr, sc = sel[rows], sel[cols]
    keep = sr & sc
    strad = sr != sc
    end = np.where(sr, rows, cols)[strad]
    passed = (vals["passed"] != 0)[strad]
    oa = np.bincount(new_of_old[end], minlength=R).astype(np.uint32)
    op = np.bincount(new_of_old[end[passed]], minlength=R).astype(np.uint32)
    out = dict(reads=R, pairs=int(keep.sum()), old_of_new=old_of_new, rows=new_of_old[rows[keep]].astype(np.int64), cols=new_of_old[cols[keep]].astype(np.int64),
               vals=vals[keep], outside_aligned=oa, outside_passed=op, split_pairs=int(strad.sum()), split_passed=int(passed.sum()), packed_bytes=0)
    if reads is not None:
        packed, off, lens = reads
        lens = np.asarray(lens, dtype=np.int64)[old_of_new]
        nb = _packed_bytes(lens)
        noff = np.concatenate([[0], np.cumsum(nb)]).astype(np.int64)
        pb = int(noff[-1])
        src = np.repeat(np.asarray(off, dtype=np.int64)[old_of_new] - noff[:-1], nb) + np.arange(pb)
        buf = np.zeros(pb + 16, dtype=np.uint8)
        buf[:pb] = np.asarray(packed, dtype=np.uint8)[src]
        last = noff[1:][(lens % 4) != 0] - 1
        buf[last] &= ((0xFF << (2 * (4 - lens[(lens % 4) != 0] % 4))) & 0xFF).astype(np.uint8)
        out.update(packed_bytes=pb, packed=buf, byte_off=noff[:-1].astype(np.uint64), len=lens.astype(np.uint32))
    return out


ARRAYS = ("old_of_new", "rows", "cols", "outside_aligned", "outside_passed")
READ_ARRAYS = ("packed", "byte_off", "len")


def same_induced(got, want, reads=True):
    """None, or the name of the first thing that differs."""
    for k in ("reads", "pairs") + (("packed_bytes",) if reads else ()):
        if int(got[k]) != int(want[k]):
            return k
    for k in ARRAYS + (READ_ARRAYS if reads and "packed" in want else ()):
        a, b = np.asarray(got[k]), np.asarray(want[k])
        if a.shape != b.shape or a.dtype != b.dtype or not (a == b).all():
            return k
    if got["vals"].tobytes() != want["vals"].tobytes():          # bit for bit, the padding byte included
        return "vals"
    return None


def strictly_ascending(rows, cols):
    rows, cols = np.asarray(rows), np.asarray(cols)
    return bool(((rows[1:] > rows[:-1]) | ((rows[1:] == rows[:-1]) & (cols[1:] > cols[:-1]))).all()) and bool((rows < cols).all())


# ---- the bad-read rule with outside counts ---------------------------------------------------------------------------------------------
def bad_reads(M, rows, cols, vals, outside_aligned=None, outside_passed=None, cutoff=0.65):
    """find_bad_reads (src/main.cpp:553-571) with the pairs the list does not hold counted in: bool[M]."""
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    passed = vals["passed"] != 0
    deg = np.bincount(rows, minlength=M) + np.bincount(cols, minlength=M)
    pas = np.bincount(rows[passed], minlength=M) + np.bincount(cols[passed], minlength=M)
    if outside_aligned is not None:
        deg = deg + np.asarray(outside_aligned, dtype=np.int64); pas = pas + np.asarray(outside_passed, dtype=np.int64)
    return (pas + 1.0) / (deg + 1.0) <= cutoff


# ---- hand cases ------------------------------------------------------------------------------------------------------------------------
def _vals(passed):
    v = np.zeros(len(passed), dtype=po.OVERLAP_DTYPE)
    v["passed"] = passed
    v["score"] = np.arange(len(passed)) + 1                         # (so that a swapped record shows)
    v["direction"] = -1; v["directionT"] = -1
    return v


def hand_cases():
    """(name, M, rows, cols, passed, part_of_read, part, claims): claims = old_of_new, kept pairs (new ids, with the input index of each),
    outside_aligned, outside_passed."""
    return [
        ("everything", 4, [0, 0, 2], [1, 3, 3], [1, 0, 1], [5, 5, 5, 5], 5, dict(old=[0, 1, 2, 3], kept=[(0, 1, 0), (0, 3, 1), (2, 3, 2)], oa=[0, 0, 0, 0], op=[0, 0, 0, 0])),
        ("nothing", 4, [0, 0, 2], [1, 3, 3], [1, 0, 1], [5, 5, 5, 5], 4, dict(old=[], kept=[], oa=[], op=[])),
        ("unassigned", 5, [0, 1, 1, 3], [1, 2, 4, 4], [1, 1, 0, 1], [-1, -1, 0, 0, 0], -1, dict(old=[0, 1], kept=[(0, 1, 0)], oa=[0, 2], op=[0, 1])),
        ("alternating", 6, [0, 0, 1, 2, 2, 4], [1, 2, 3, 3, 4, 5], [0, 1, 1, 0, 1, 0], [1, 0, 1, 0, 1, 0], 1,
         dict(old=[0, 2, 4], kept=[(0, 1, 1), (1, 2, 4)], oa=[1, 1, 1], op=[0, 0, 0])),
        # the issue's read: one passed pair inside, three failed pairs out of the part — (1 + 1) / (4 + 1) in the whole run, (1 + 1) / (1 + 1) alone
        ("planted", 6, [0, 0, 0, 0], [1, 2, 3, 4], [1, 0, 0, 0], [7, 7, 3, 3, 2, 2], 7, dict(old=[0, 1], kept=[(0, 1, 0)], oa=[3, 0], op=[0, 0])),
        ("negative_part", 3, [0, 1], [1, 2], [1, 1], [-2147483648, -2147483648, 2147483647], -2147483648, dict(old=[0, 1], kept=[(0, 1, 0)], oa=[0, 1], op=[0, 1])),
    ]


def case_input(case):
    name, M, rows, cols, passed, part_of_read, part, claims = case
    return M, np.array(rows, dtype=np.int64), np.array(cols, dtype=np.int64), _vals(passed), np.array(part_of_read, dtype=np.int32), part


def check_case(case, got):
    claims = case[-1]
    vals = _vals(case[4])
    assert got["old_of_new"].tolist() == claims["old"], case[0]
    assert list(zip(got["rows"].tolist(), got["cols"].tolist())) == [(r, c) for r, c, _ in claims["kept"]], case[0]
    assert got["vals"].tobytes() == vals[[a for _, _, a in claims["kept"]]].tobytes() if claims["kept"] else len(got["vals"]) == 0, case[0]
    assert got["outside_aligned"].tolist() == claims["oa"] and got["outside_passed"].tolist() == claims["op"], case[0]


# ---- multi-component inputs ------------------------------------------------------------------------------------------------------------
def _failed(rng, n, L):
    v = np.zeros(n, dtype=po.OVERLAP_DTYPE)
    v["direction"] = -1; v["directionT"] = -1
    v["begQ"] = rng.integers(0, L // 2 + 1, n); v["endQ"] = v["begQ"] + rng.integers(0, L // 2 + 1, n)
    v["begT"] = rng.integers(0, L // 2 + 1, n); v["endT"] = v["begT"] + rng.integers(0, L // 2 + 1, n)
    v["score"] = rng.integers(0, L, n); v["rc"] = rng.integers(0, 2, n)
    return v


def build_input(seed, blocks, L=64, cov=6, n_failed=0, plant=True, lone=0, reads=True, p_nodir=0.02):
    """Several graphs side by side.  blocks = (("layout", m) | ("random", m), ...): sg.layout_overlaps (reads of L bases at coverage cov,
    jitter 0, so that every suffix is a valid prefix of a read of L bases and contigs can be generated) or sg.random_overlaps on m reads,
    each on an id range of its own; `lone` reads without a pair; n_failed failed pairs between reads of different blocks; with plant a
    block of two reads (x, y) with one passed pair, x with three failed pairs into three other blocks — x is bad in the whole graph at
    cutoff 0.65 ((1 + 1) / (4 + 1)) and good in any part that holds whole blocks without the outside counts.  Ids are then interleaved by
    a random permutation (sg.relabel).  p_nodir is layout_overlaps': pairs with one direction only leave S with one image of a pair, on
    which the chains of the contig stage are not a function of S alone — inputs whose contigs are compared take p_nodir = 0.  Returns dict(M, rows, cols, vals, block (i32[M]: the block of every read), planted (the id of x
    or -1), reads = (packed, off, lens) with every read L bases long (random bases, random low bits in last bytes) or None)."""
    rng = np.random.default_rng(seed)
    rr, cc, vv, block = [], [], [], []
    base = 0
    for b, (kind, m) in enumerate(blocks):
        if kind == "layout":
            r, c, v = sg.layout_overlaps(rng, m, cov, L=L, jitter=0, p_nodir=p_nodir)
            for f in ("endQ", "endT"):
                v[f] = np.minimum(v[f], L)
        else:
            r, c, v = sg.random_overlaps(rng, m, density=min(1.0, 6.0 / max(m, 1)))
        rr.append(r + base); cc.append(c + base); vv.append(v); block += [b] * m
        base += m
    nb = len(blocks)
    planted = -1
    if plant:
        assert nb >= 3
        x = base
        v = np.zeros(1, dtype=po.OVERLAP_DTYPE)
        v["passed"] = 1; v["direction"] = 2; v["directionT"] = 1; v["suffix"] = L // 4; v["suffixT"] = L // 4
        v["endQ"] = L; v["begQ"] = L // 4; v["endT"] = L - L // 4; v["score"] = L - L // 4
        rr.append(np.array([x])); cc.append(np.array([x + 1])); vv.append(v); block += [nb, nb]
        starts = np.concatenate([[0], np.cumsum([m for _, m in blocks])])
        tgt = np.array([int(rng.integers(starts[b], starts[b + 1])) for b in rng.choice(nb, 3, replace=False)], dtype=np.int64)
        rr.append(tgt); cc.append(np.full(3, x)); vv.append(_failed(rng, 3, L))
        planted = x
        base += 2
    block += list(range(nb + 1, nb + 1 + lone))
    M = base + lone
    block = np.array(block, dtype=np.int32)
    if n_failed:
        u, w = rng.integers(0, base, 4 * n_failed), rng.integers(0, base, 4 * n_failed)
        ok = block[u] != block[w]
        u, w = np.minimum(u, w)[ok], np.maximum(u, w)[ok]
        key = np.unique(u * M + w)
        if plant:
            key = key[(key // M != planted) & (key % M != planted)]       # (x keeps exactly its three)
        key = key[:n_failed]
        rr.append(key // M); cc.append(key % M); vv.append(_failed(rng, len(key), L))
    rows, cols, vals = np.concatenate(rr), np.concatenate(cc), np.concatenate(vv)
    lo, hi = np.minimum(rows, cols), np.maximum(rows, cols)
    flip = rows > cols
    if flip.any():
        t = sg.transpose(vals[flip]); vals = vals.copy(); vals[flip] = t
    perm = rng.permutation(M)
    rows, cols, vals = sg.relabel(perm, lo, hi, vals)
    assert strictly_ascending(rows, cols)
    inv = np.empty(M, dtype=np.int64); inv[perm] = np.arange(M)
    out = dict(M=M, rows=rows, cols=cols, vals=vals, block=block[inv], planted=int(perm[planted]) if planted >= 0 else -1, reads=None, L=L)
    if reads:
        nbytes = (L + 3) // 4
        packed = rng.integers(0, 256, M * nbytes + 16).astype(np.uint8); packed[-16:] = 0
        out["reads"] = (packed, (np.arange(M, dtype=np.uint64) * np.uint64(nbytes)), np.full(M, L, dtype=np.uint32))
    return out


# ---- the late stages, whole and by parts -----------------------------------------------------------------------------------------------
def late_stages(e, M, cutoff=0.65, fuzz=0, simplify=(3, 4), place=True, contigs=True):
    """What the tests compare, from an engine that holds reads and a loaded edge list: flags, S, contigs under flags 0 .. 3, the component
    labels of S, then simplify_graph and the contigs, placements and component labels behind it."""
    out = dict(M=M, stats=e.transitive_reduction(cutoff, fuzz))
    out["flags"] = e.export_read_flags(M)
    out["S"] = e.export_string_graph()
    out["contigs"] = []
    for fl in range(4 if contigs else 0):
        e.generate_contigs(circular=bool(fl & 1), singletons=bool(fl & 2))
        out["contigs"].append(e.export_contigs())
    out["comp"] = e.graph_components("string")[0]["comp_of_read"]
    if simplify is not None:
        e.simplify_graph(*simplify)
        out["flags_clean"] = e.export_read_flags(M)
        out["S_clean"] = e.export_string_graph()
        e.generate_contigs(circular=True, singletons=True)
        out["contigs_clean"] = e.export_contigs()
        out["comp_clean"] = e.graph_components("string")[0]["comp_of_read"]
        if place:
            out["placements"] = e.place_reads()[0]
    return out


def _same_s(part_s, whole_s, old_of_new, new_of_old, sel):
    keep = sel[whole_s["rows"]] & sel[whole_s["cols"]]
    if part_s["n"] != int(keep.sum()):
        return "S count"
    if not ((part_s["rows"] == new_of_old[whole_s["rows"][keep]]).all() and (part_s["cols"] == new_of_old[whole_s["cols"][keep]]).all()):
        return "S ids"
    for f in FIELDS:
        if not (part_s["vals"][f] == whole_s["vals"][f][keep]).all():
            return "S " + f
    return None


def _chains(c, ids=None):
    out = []
    for k in range(c["n"]):
        a, b = int(c["chain_off"][k]), int(c["chain_off"][k + 1])
        r = c["chain_read"][a:b]
        out.append((tuple((r if ids is None else ids[r]).tolist()), tuple(c["chain_prefix"][a:b].tolist()), tuple(c["chain_strand"][a:b].tolist()), c["seqs"][k], int(c["kinds"][k])))
    return out


def _same_contigs(part_c, whole_c, old_of_new, sel):
    want = [x for x in _chains(whole_c) if sel[x[0][0]]]
    got = _chains(part_c, old_of_new)
    if got == want:
        return None
    if len(got) != len(want):
        return "contigs (%d against %d)" % (len(got), len(want))
    k = next(i for i in range(len(got)) if got[i] != want[i])
    f = next(i for i in range(5) if got[k][i] != want[k][i])
    return "contig %d of %d, %s: %r against %r" % (k, len(got), ("reads", "prefixes", "strands", "sequence", "kind")[f], got[k][f], want[k][f])


def _same_placements(part, whole, old_of_new, sel):
    pp, wp = part["placements"]["reads"], whole["placements"]["reads"][old_of_new]
    for f in ("start", "score", "strand", "kind", "flags"):
        if not (pp[f] == wp[f]).all():
            return "placements " + f
    anch = pp["kind"] == 2
    if not (old_of_new[pp["anchor"][anch]] == wp["anchor"][anch]).all():
        return "placements anchor"
    first_p = old_of_new[part["contigs_clean"]["chain_read"][part["contigs_clean"]["chain_off"][:-1]]] if part["contigs_clean"]["n"] else np.zeros(0, np.int64)
    first_w = whole["contigs_clean"]["chain_read"][whole["contigs_clean"]["chain_off"][:-1]] if whole["contigs_clean"]["n"] else np.zeros(0, np.int64)
    on = pp["contig"] >= 0
    if not ((wp["contig"] >= 0) == on).all() or not (first_p[pp["contig"][on]] == first_w[wp["contig"][on]]).all():
        return "placements contig"
    mine = np.flatnonzero(sel[first_w]) if len(first_w) else np.zeros(0, np.int64)
    for f in ("credited_reads", "credited_bases"):
        if not (part["placements"][f] == whole["placements"][f][mine]).all():
            return "placements " + f
    return None


def _same_components(part_comp, whole_comp, old_of_new):
    """Components are numbered by ascending smallest read and the numbering of the reads is monotone: the part's labels are the whole
    run's, restricted and ranked."""
    return bool((np.unique(whole_comp[old_of_new], return_inverse=True)[1] == part_comp).all())


def compare_part(part, whole, old_of_new):
    """None, or what differs first between a part's late stages and the whole run's restricted to the part."""
    M = whole["M"]
    old_of_new = np.asarray(old_of_new, dtype=np.int64)
    sel = np.zeros(M, dtype=bool); sel[old_of_new] = True
    new_of_old = np.cumsum(sel) - 1
    if not (part["flags"] == whole["flags"][old_of_new]).all():
        return "flags"
    bad = _same_s(part["S"], whole["S"], old_of_new, new_of_old, sel)
    if bad:
        return bad
    for fl in range(len(whole["contigs"])):
        bad = _same_contigs(part["contigs"][fl], whole["contigs"][fl], old_of_new, sel)
        if bad:
            return "flags %d: %s" % (fl, bad)
    if not _same_components(part["comp"], whole["comp"], old_of_new):
        return "components"
    if "S_clean" in whole:
        if not (part["flags_clean"] == whole["flags_clean"][old_of_new]).all():
            return "flags after simplify_graph"
        bad = _same_s(part["S_clean"], whole["S_clean"], old_of_new, new_of_old, sel) or _same_contigs(part["contigs_clean"], whole["contigs_clean"], old_of_new, sel)
        if bad:
            return "after simplify_graph: " + bad
        if not _same_components(part["comp_clean"], whole["comp_clean"], old_of_new):
            return "components after simplify_graph"
        if "placements" in whole:
            bad = _same_placements(part, whole, old_of_new, sel)
            if bad:
                return bad
    return None


def assemble_by_parts(engine, nparts, second, M, min_reads=1, outside=True, cutoff=0.65, fuzz=0, simplify=(3, 4), place=True, device=False, contigs=True):
    """The driver.  `engine` holds the whole input (reads and the loaded edge list); the overlaps graph is partitioned into nparts parts,
    every part (and -1 when reads stay unassigned) is cut out with induce_part, loaded into `second` and run through late_stages.
    device: the pairs and the counts go through the device views (set_overlaps_device / set_outside_counts_device: copied device to device),
    the reads through the host copies (set_reads_device borrows its arrays, and the views die with the next induce_part).
    Returns [(part, induced dict, induce stats, late_stages dict)]."""
    part_of_read, weight = engine.partition_components(nparts, graph="overlaps", min_reads=min_reads, nreads=M)
    out = []
    for p in ([-1] if (part_of_read < 0).any() else []) + list(range(nparts)):
        ind, st = engine.induce_part(part_of_read, p)
        if ind["reads"] == 0:                                        # (more parts than components: nothing to assemble)
            out.append((p, ind, st, None))
            continue
        if device:
            second.set_reads(ind["packed"], ind["byte_off"], ind["len"])
            second.set_overlaps_device(ind["reads"], ind["d_rows"], ind["d_cols"], ind["d_vals"], ind["pairs"])
            if outside:
                second.set_outside_counts_device(ind["reads"], ind["d_outside_aligned"], ind["d_outside_passed"])
        else:
            second.load_part(ind, outside=outside)
        out.append((p, ind, st, late_stages(second, ind["reads"], cutoff, fuzz, simplify, place, contigs)))
    return part_of_read, out
