"""CPU: the grammar of elba_set_reads_text as tests/text_index_util.py restates it — the literal loop and the vectorised form agree with
each other, with the hand cases, and with fasta.write_fai on the FASTA encoder's boundary grid; the local line-shape rule is the shape it
claims to be; write_fai_from_index round-trips; and the library, the header and the binding carry the new entry points."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import elba_amd
from elba_amd import capi, fasta
import prim_util as pu
import text_index_util as tx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _triples(idx):
    return [(int(r["len"]), int(r["pos"]), int(r["bases"])) for r in idx["recs"]]


@pytest.mark.parametrize("case", tx.GOOD_CASES, ids=[c[0] for c in tx.GOOD_CASES])
def test_hand_cases_give_their_claimed_records_in_both_forms(case):
    _, data, fmt, recs, names = case
    for fn in (tx.index_loop, tx.index_numpy):
        idx = fn(data, fmt)
        assert _triples(idx) == recs and tx.names_of(data, idx) == names, fn.__name__
    # the same text at a file offset: pos and name_pos carry it, nothing else moves
    a, b = tx.index_numpy(data, fmt), tx.index_numpy(data, fmt, (1 << 40) + 5)
    assert (b["recs"]["pos"] - a["recs"]["pos"] == (1 << 40) + 5).all() and (b["name_pos"] - a["name_pos"] == (1 << 40) + 5).all()
    assert (a["recs"]["len"] == b["recs"]["len"]).all() and (a["recs"]["bases"] == b["recs"]["bases"]).all() and (a["name_len"] == b["name_len"]).all()
    assert tx.same_index(tx.index_loop(data, fmt, (1 << 40) + 5), b)


@pytest.mark.parametrize("case", tx.BAD_CASES, ids=[c[0] for c in tx.BAD_CASES])
def test_error_cases_are_rejected_by_both_forms_with_the_same_kind_and_offset(case):
    _, data, fmt, kind, off = case
    assert tx.error_of(tx.index_loop, data, fmt) == (kind, off)
    assert tx.error_of(tx.index_numpy, data, fmt) == (kind, off)
    assert tx.error_of(tx.index_numpy, data, fmt, 1000) == (kind, off + 1000) == tx.error_of(tx.index_loop, data, fmt, 1000)


def test_local_rule_is_the_line_shape():
    """every list of up to six line lengths in 0 .. 3: the per-line rule holds exactly when the lengths read bases, .., bases, t, 0, .., 0"""
    for k in range(7):
        for ll in itertools.product(range(4), repeat=k):
            assert tx.local_rule_holds(list(ll)) == tx.shape_holds(list(ll)), ll


def test_forms_agree_on_random_texts():
    """random FASTA and FASTQ, good and broken: the same records or the same (kind, offset)"""
    rng = np.random.default_rng(11)
    seen = set()
    for it in range(900):
        lens = rng.integers(0, 30, int(rng.integers(0, 7)))
        seqs = tx.random_seqs(rng, lens)
        final = bool(rng.integers(0, 2))
        if it % 2:
            data = bytearray(tx.fastq_bytes(seqs, final_newline=final))
        else:
            data = bytearray(tx.fasta_bytes(seqs, int(rng.integers(0, 9)), final_newline=final))
        if it % 3 and len(data) > 2:      # break it: overwrite, insert or delete a byte
            at = int(rng.integers(0, len(data)))
            what = int(rng.integers(0, 3))
            if what == 0:
                data[at] = int(rng.choice(np.frombuffer(b"\n\r>@+A ", dtype=np.uint8)))
            elif what == 1:
                data.insert(at, int(rng.choice(np.frombuffer(b"\n\r>@+A", dtype=np.uint8))))
            else:
                del data[at]
        data = bytes(data)
        for fmt in ("auto", "fasta", "fastq"):
            e1, e2 = tx.error_of(tx.index_loop, data, fmt), tx.error_of(tx.index_numpy, data, fmt)
            assert e1 == e2, (data, fmt, e1, e2)
            seen.add(e1[0] if e1 else None)
            if e1 is None:
                assert tx.same_index(tx.index_loop(data, fmt), tx.index_numpy(data, fmt)), (data, fmt)
    assert {None, tx.CR, tx.SHAPE, tx.FQ_LINES, tx.FQ_AT, tx.FQ_PLUS, tx.FQ_QUAL} <= seen


@pytest.mark.parametrize("width", pu.INGEST_WIDTHS)
def test_fasta_form_equals_write_fai_on_the_ingest_grid(tmp_path, width):
    """INGEST_WIDTHS x INGEST_LENGTHS, with and without a final newline, forward (the last record is the empty one) and reversed"""
    seqs = pu.ingest_grid_seqs(width + 1)
    p = str(tmp_path / "grid.fa")
    for order, final in ((seqs, True), (seqs, False), (seqs[::-1], True), (seqs[::-1], False)):
        pu.write_fasta(p, order, width, final_newline=final)
        data = open(p, "rb").read()
        fasta.write_fai(p)
        names, recs = fasta.read_fai(p + ".fai")
        idx = tx.index_numpy(data)
        assert len(recs) == len(order) == len(idx["recs"])
        for f in ("len", "pos", "bases"):
            assert (idx["recs"][f] == recs[f]).all(), f
        assert tx.names_of(data, idx) == names
        assert tx.sequences_of(data, idx) == list(order)
    # the literal loop on one file of the four (it walks every byte in Python)
    assert tx.same_index(tx.index_loop(data), idx)


def test_fastq_and_fasta_of_the_same_reads_index_the_same_bases():
    rng = np.random.default_rng(5)
    seqs = tx.random_seqs(rng, [0, 1, 5, 70, 0, 33])
    fa, fq = tx.fasta_bytes(seqs, 60), tx.fastq_bytes(seqs)
    assert tx.sequences_of(fa, tx.index_numpy(fa)) == seqs == tx.sequences_of(fq, tx.index_numpy(fq))
    assert tx.names_of(fa, tx.index_numpy(fa)) == tx.names_of(fq, tx.index_numpy(fq)) == ["read%d" % i for i in range(6)]


def test_write_fai_from_index_round_trips_through_read_fai(tmp_path):
    data = tx.fasta_bytes(tx.random_seqs(np.random.default_rng(3), [100, 0, 61, 7]), 60)
    idx = tx.index_numpy(data, file_off=12345)
    names = tx.names_of(data, idx, 12345)
    p = fasta.write_fai_from_index(names, idx["recs"], str(tmp_path / "x.fai"))
    names2, recs2 = fasta.read_fai(p)
    assert names2 == names and recs2.dtype == fasta.FAI_DTYPE and (recs2 == idx["recs"]).all()
    for line, r in zip(open(p), idx["recs"]):
        t = line.split("\t")
        assert len(t) == 5 and int(t[4]) == int(r["bases"]) + 1


def test_library_header_and_binding_carry_the_text_entry_points():
    """fails without the feature: the two symbols, their declarations, the binding's list and the three Engine methods"""
    L = elba_amd.load_library()
    new = ["elba_set_reads_text", "elba_export_read_index"]
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "elba_amd.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(elba_[a-z0-9_]+)\s*\(", hdr))
    for n in new:
        assert hasattr(L, n), n
        assert n in capi.EXPORTED_SYMBOLS and n in declared, n
    assert L.elba_abi_version() == 3
    for m in ("set_reads_text", "export_read_index", "set_reads_file"):
        assert callable(getattr(elba_amd.Engine, m, None)), m
    assert C.sizeof(capi.TextCfg) == 16 and C.sizeof(capi.TextStats) == 5 * 8 + 2 * 4 + 3 * 4 + 4      # (4: tail padding to the struct's 8-byte alignment)
    assert "no device inflate" in elba_amd.Engine.set_reads_file.__doc__
    assert L.elba_set_reads_text(None, None, 0, 0, None, None) == 1 and L.elba_export_read_index(None, None, None, None, 0) == 1
