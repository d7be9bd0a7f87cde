// state.hpp — which products of a context are valid, and what every mutating entry point does to that.  This table is the ONE place
// that decides it: a stage names its event at three points (enter / accepted / done) and asks has(); nothing else touches validity.
// Plain C++17, no HIP: elba_amd/hostcpp/test_state_table.cpp compiles it alone and tests/state_cases.py holds what it must answer.
#pragma once
#include <cstdint>

namespace elba {

enum Product : unsigned {
    P_READS,        // the context's own reads (elba_set_reads*, elba_adopt_trimmed_reads)
    P_COUNTS,       // reliable k-mers and their columns
    P_A,            // the k-mer matrix
    P_B,            // the seed matrix
    P_ALN,          // alignments of B's pairs
    P_EDGES,        // an edge list loaded with elba_set_overlaps or left by elba_prune_reads: while valid it is the string graph's input, not P_ALN
    P_S,            // the string graph
    P_CONTIGS,      // contigs; they are those of the current graph only while P_S is valid too (exports and contig_* stats ask for both)
    P_PILEUP,       // pileup of the graph's input
    P_TRIM,         // trimmed reads: a snapshot in buffers of its own
    P_COUNT
};

using Mask = uint16_t;
template <class... P> constexpr Mask mask(P... p) { return (Mask)((0u | ... | (1u << p))); }

struct Validity { Mask bits = 0; };

enum Event : unsigned {
    EV_SET_READS, EV_SET_READS_FASTA, EV_SET_READS_DEVICE, EV_ADOPT_TRIMMED_READS, EV_MATRIX_OF_OLD_READS,
    EV_COUNT_KMERS, EV_CREATE_KMER_MATRIX, EV_SET_KMER_MATRIX, EV_SET_KMER_MATRIX_DEVICE, EV_DIST_COUNT_RECORDS, EV_DIST_SET_PANEL,
    EV_CREATE_SEED_MATRIX, EV_SEED_MATRIX_BEGIN, EV_SEED_MATRIX_END, EV_SEED_MATRIX_SEND, EV_SEED_MATRIX_RECV,
    EV_ALIGN_SEEDS, EV_DIST_SET_ALL_READS, EV_SET_OVERLAPS, EV_TRANSITIVE_REDUCTION, EV_RESOLVE_STARS, EV_CLIP_TIPS, EV_POP_BUBBLES, EV_CUT_WEAK_OVERLAPS, EV_CUT_BRIDGES,
    EV_GENERATE_CONTIGS,
    EV_READ_PILEUP, EV_PRUNE_READS, EV_TRIM_READS,
    EV_COUNT
};

// One row per event.  A call drops `enter` before it looks at anything (whatever it ends in), `accepted` once its state and
// arguments have passed, `done` when it has succeeded, and then publishes `publish`.  `of_aln` is dropped with `accepted` unless a
// loaded edge list is valid: a graph built from P_EDGES (and its contigs) does not come from this context's matrices or alignments.
// The table is per event, not a dependency closure: a new pileup drops the trimmed reads, but elba_prune_reads and elba_align_seeds
// drop the pileup and leave the trimmed reads, which are a snapshot.
struct Row { Event ev; const char *name; Mask enter, accepted, done, publish, of_aln; };

// what a new read set drops (P_CONTIGS is not among them: without P_S nothing reads it, and the next reduction drops it)
constexpr Mask OF_READS = mask(P_COUNTS, P_ALN, P_EDGES, P_S, P_PILEUP, P_TRIM);
// what a call that replaces A or B drops besides the matrices: the alignments of the old B and the pileup — and, in `of_aln`, the graph
constexpr Mask OF_B = mask(P_ALN, P_PILEUP), GRAPH = mask(P_S, P_CONTIGS);

constexpr Row TABLE[] = {
    // event                         name                          enter                    accepted                              done                              publish         of_aln
    {EV_SET_READS,              "set_reads",              0,                       0,                                    OF_READS,                         mask(P_READS),  0},
    {EV_SET_READS_FASTA,        "set_reads_fasta",        mask(P_PILEUP, P_TRIM),  0,                                    OF_READS,                         mask(P_READS),  0},      // (the only one of the four that drops something when it is rejected)
    {EV_SET_READS_DEVICE,       "set_reads_device",       0,                       0,                                    OF_READS,                         mask(P_READS),  0},
    {EV_ADOPT_TRIMMED_READS,    "adopt_trimmed_reads",    0,                       0,                                    OF_READS,                         mask(P_READS),  0},      // (consumes P_TRIM: its buffers become the reads)
    // follows each of the four above when A was built from the old reads (Ctx::A_has_kmers); an A handed over as triples or a panel stays
    {EV_MATRIX_OF_OLD_READS,    "matrix_of_old_reads",    0,                       0,                                    mask(P_A, P_B),                   0,              0},
    {EV_COUNT_KMERS,            "count_kmers",            0,                       mask(P_COUNTS, P_A, P_B) | OF_B,      0,                                mask(P_COUNTS), GRAPH},
    {EV_CREATE_KMER_MATRIX,     "create_kmer_matrix",     0,                       mask(P_A, P_B) | OF_B,                0,                                mask(P_A),      GRAPH},
    // the triples land in the buffers the counted columns live in: the counts go too (also on an owner of exchanged records, whose columns
    // are in buffers of their own and would survive: such a context takes panels, not triples, and the row stays unconditional)
    {EV_SET_KMER_MATRIX,        "set_kmer_matrix",        0,                       mask(P_COUNTS, P_A, P_B) | OF_B,      0,                                mask(P_A),      GRAPH},
    {EV_SET_KMER_MATRIX_DEVICE, "set_kmer_matrix_device", 0,                       mask(P_COUNTS, P_A, P_B) | OF_B,      0,                                mask(P_A),      GRAPH},      // (accepted before the device checks the indices)
    {EV_DIST_COUNT_RECORDS,     "dist_count_records",     0,                       mask(P_COUNTS, P_A, P_B) | OF_B,      0,                                mask(P_COUNTS), GRAPH},      // (the owner's columns leave A for buffers of their own)
    {EV_DIST_SET_PANEL,         "dist_set_panel",         0,                       mask(P_A, P_B) | OF_B,                0,                                mask(P_A),      GRAPH},      // (P_COUNTS stays: an owner's counted columns are in buffers of their own)
    {EV_CREATE_SEED_MATRIX,     "create_seed_matrix",     0,                       mask(P_B) | OF_B,                     0,                                mask(P_B),      GRAPH},
    {EV_SEED_MATRIX_BEGIN,      "seed_matrix_begin",      0,                       mask(P_B) | OF_B,                     0,                                0,              GRAPH},      // (B stays invalid until _end)
    {EV_SEED_MATRIX_END,        "seed_matrix_end",        0,                       0,                                    0,                                mask(P_B),      0},          // (_begin dropped what depends on B, and nothing can align in between)
    {EV_SEED_MATRIX_SEND,       "seed_matrix_send",       0,                       mask(P_B) | OF_B,                     0,                                0,              GRAPH},
    {EV_SEED_MATRIX_RECV,       "seed_matrix_recv",       0,                       0,                                    0,                                mask(P_B),      0},          // (a step to be repeated, ELBA_ERR_RETRY, is not done)
    // fresh alignments replace a loaded edge list as the graph's input; P_CONTIGS and P_TRIM stay (no P_S: nothing reads the contigs)
    {EV_ALIGN_SEEDS,            "align_seeds",            mask(P_PILEUP),          mask(P_ALN, P_EDGES, P_S),            0,                                mask(P_ALN),    0},
    // the replicated reads are what a row shard aligns: its alignments go, and only when the call succeeds.  An S computed from them stays
    {EV_DIST_SET_ALL_READS,     "dist_set_all_reads",     mask(P_PILEUP, P_TRIM),  0,                                    mask(P_ALN),                      0,              0},
    {EV_SET_OVERLAPS,           "set_overlaps",           mask(P_PILEUP),          mask(P_EDGES, P_S),                   0,                                mask(P_EDGES),  0},          // (P_CONTIGS and P_TRIM stay, as after align_seeds)
    {EV_TRANSITIVE_REDUCTION,   "transitive_reduction",   mask(P_CONTIGS),         mask(P_S),                            0,                                mask(P_S),      0},
    // S is invalid while the rounds are queued and valid again when the counters are back; accepted only after every buffer is
    // reserved, so that a rejected cfg — or no memory — leaves S and the contigs as they are
    {EV_RESOLVE_STARS,          "resolve_stars",          0,                       mask(P_S, P_CONTIGS),                 0,                                mask(P_S),      0},          // (as clip_tips, row for row: it removes reads; it stands here because the four rows below follow one another)
    {EV_CLIP_TIPS,              "clip_tips",              0,                       mask(P_S, P_CONTIGS),                 0,                                mask(P_S),      0},
    {EV_POP_BUBBLES,            "pop_bubbles",            0,                       mask(P_S, P_CONTIGS),                 0,                                mask(P_S),      0},          // (as clip_tips, row for row)
    {EV_CUT_WEAK_OVERLAPS,      "cut_weak_overlaps",      0,                       mask(P_S, P_CONTIGS),                 0,                                mask(P_S),      0},          // (the same: it removes entries, not reads, which the table does not see)
    {EV_CUT_BRIDGES,            "cut_bridges",            0,                       mask(P_S, P_CONTIGS),                 0,                                mask(P_S),      0},          // (as clip_tips, row for row: it removes reads)
    {EV_GENERATE_CONTIGS,       "generate_contigs",       mask(P_CONTIGS),         0,                                    0,                                mask(P_CONTIGS), 0},         // (elba_generate_contigs and _ex: a rejected call leaves no contigs)
    {EV_READ_PILEUP,            "read_pileup",            mask(P_PILEUP, P_TRIM),  0,                                    0,                                mask(P_PILEUP), 0},          // (the trimmed reads are cut from the pileup they were asked of)
    // the kept pairs become the loaded edge list; the alignments and the trimmed reads stay
    {EV_PRUNE_READS,            "prune_reads",            0,                       0,                                    mask(P_S, P_CONTIGS, P_PILEUP),   mask(P_EDGES),  0},
    {EV_TRIM_READS,             "trim_reads",             mask(P_TRIM),            0,                                    0,                                mask(P_TRIM),   0},
};

constexpr bool table_in_order()
{
    if (sizeof(TABLE) / sizeof(TABLE[0]) != EV_COUNT) return false;
    for (unsigned e = 0; e < EV_COUNT; ++e) if (TABLE[e].ev != e) return false;
    return true;
}
static_assert(table_in_order(), "state.hpp: TABLE needs one row per Event, in the enum's order");

template <class... P> constexpr bool has(Validity v, P... p) { return (v.bits & mask(p...)) == mask(p...); }      // every one of them
constexpr void enter(Validity &v, Event e) { v.bits &= (Mask)~TABLE[e].enter; }
constexpr void accepted(Validity &v, Event e) { v.bits &= (Mask)~(TABLE[e].accepted | (has(v, P_EDGES) ? 0 : TABLE[e].of_aln)); }
constexpr void done(Validity &v, Event e) { v.bits = (Mask)((v.bits & ~TABLE[e].done) | TABLE[e].publish); }

}  // namespace elba
