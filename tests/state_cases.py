"""What a context holds valid after every call of a sequence (elba_amd/csrc/state.hpp), as data: tests/test_state_cpu.py walks the table
program through every case, tests/test_gpu_state.py walks an Engine through those a GPU can act out and probes its exports.

A step is (call, valid products after it).  A call is an event of the table, plain (it succeeds) or with an ending:
  :reject  its arguments are refused                     :state  good arguments, refused for what the context holds
  :fail    it fails after its checks have passed (no GPU test can stage that)
"matrix_of_old_reads" is no call: it is what a new read set does to an A that was built from the old one, and follows the call at once.

tightening: the case shows one of the places where a call now drops more than it used to (a matrix replaced under alignments, the contig
counters); every other case holds for the code before the table as well, by its exports."""

PRODUCTS = ("reads", "counts", "A", "B", "aln", "edges", "S", "contigs", "pileup", "trim")

# through the first contigs; FULL's last state is every product but a loaded edge list
ALIGNED = [
    ("set_reads", "reads"),
    ("count_kmers", "reads counts"),
    ("create_kmer_matrix", "reads counts A"),
    ("create_seed_matrix", "reads counts A B"),
    ("align_seeds", "reads counts A B aln"),
]
PILED = ALIGNED + [
    ("read_pileup", "reads counts A B aln pileup"),
    ("trim_reads", "reads counts A B aln pileup trim"),
]
FULL = PILED + [
    ("transitive_reduction", "reads counts A B aln S pileup trim"),
    ("generate_contigs", "reads counts A B aln S contigs pileup trim"),
]

CASES = {
    "straight_pipeline_through_adopt": dict(steps=FULL + [
        ("adopt_trimmed_reads", "reads A B contigs"),              # (the contigs' bit outlives S; nothing reads it without S)
        ("matrix_of_old_reads", "reads contigs"),
        ("count_kmers", "reads counts"),
    ]),
    "prune_then_reduce_then_contigs": dict(steps=PILED + [
        ("prune_reads", "reads counts A B aln edges trim"),       # the pileup goes, the trimmed reads stay
        ("transitive_reduction", "reads counts A B aln edges S trim"),
        ("generate_contigs", "reads counts A B aln edges S contigs trim"),
    ]),
    "reentry_by_set_overlaps": dict(steps=FULL + [
        ("set_overlaps", "reads counts A B aln edges contigs trim"),
        ("transitive_reduction", "reads counts A B aln edges S trim"),
        ("generate_contigs", "reads counts A B aln edges S contigs trim"),
    ]),
    "reentry_by_set_reads": dict(steps=FULL + [
        ("set_reads", "reads A B contigs"),
        ("matrix_of_old_reads", "reads contigs"),
        ("count_kmers", "reads counts"),
        ("create_kmer_matrix", "reads counts A"),
    ]),
    "rejected_calls_differ": dict(steps=FULL + [
        ("clip_tips:reject", "reads counts A B aln S contigs pileup trim"),          # leaves everything
        ("generate_contigs:reject", "reads counts A B aln S pileup trim"),           # leaves no contigs
        ("generate_contigs", "reads counts A B aln S contigs pileup trim"),
        ("trim_reads:reject", "reads counts A B aln S contigs pileup"),              # leaves no trimmed reads
        ("trim_reads", "reads counts A B aln S contigs pileup trim"),
        ("read_pileup:reject", "reads counts A B aln S contigs"),                    # leaves neither pileup nor trimmed reads
        ("clip_tips", "reads counts A B aln S"),                                     # S changed under the contigs
    ]),
    "align_after_pileup_and_trim": dict(steps=PILED + [
        ("align_seeds", "reads counts A B aln trim"),                                # the pileup goes, the trimmed reads stay
    ]),
    "clip_tips_in_flight": dict(gpu=False, steps=FULL + [
        ("clip_tips:fail", "reads counts A B aln pileup trim"),                      # no S rather than one in the wrong buffer
    ]),
    "sharded_multiplication": dict(gpu=False, steps=[
        ("dist_count_records", "counts"),
        ("dist_set_panel", "counts A"),
        ("dist_set_all_reads", "counts A"),
        ("seed_matrix_send", "counts A"),
        ("seed_matrix_recv", "counts A B"),
        ("align_seeds", "counts A B aln"),
        ("set_reads_fasta:reject", "counts A B aln"),
        ("seed_matrix_begin", "counts A"),                                           # B is invalid until _end, and its alignments go with it
        ("seed_matrix_end", "counts A B"),
        ("align_seeds", "counts A B aln"),
        ("dist_set_all_reads", "counts A B"),
    ]),
    # ---- the tightenings ----
    "reentry_by_set_kmer_matrix": dict(tightening=True, steps=FULL + [
        ("set_kmer_matrix", "reads A trim"),                       # alignments, pileup, graph and contigs of the old matrix go; so do the counts
        ("transitive_reduction:state", "reads A trim"),
        ("read_pileup:state", "reads A"),
    ]),
    "set_kmer_matrix_under_a_loaded_edge_list": dict(tightening=True, steps=FULL + [
        ("set_overlaps", "reads counts A B aln edges contigs trim"),
        ("transitive_reduction", "reads counts A B aln edges S trim"),
        ("generate_contigs", "reads counts A B aln edges S contigs trim"),
        ("set_kmer_matrix", "reads A edges S contigs trim"),       # the graph of the loaded edges does not come from the matrices
    ]),
    "recount_under_alignments": dict(tightening=True, steps=FULL + [
        ("count_kmers", "reads counts trim"),
        ("transitive_reduction:state", "reads counts trim"),
    ]),
    "contig_counters_follow_the_exports": dict(tightening=True, steps=FULL + [
        ("set_reads", "reads A B contigs"),
        ("matrix_of_old_reads", "reads contigs"),                  # no S: elba_get_stat("contig_count") is 0, as the exports refuse
    ]),
}
