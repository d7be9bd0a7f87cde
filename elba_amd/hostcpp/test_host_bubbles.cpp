// test_host_bubbles.cpp — reads -> A -> B -> PairwiseAlignment -> TransitiveReduction -> PopBubbles -> GenerateContigs, written against
// elba_host.hpp; the host copy of the popped S is held against the unpopped one on the host: it must be its entries without those of
// the popped reads, in order.
// Prints one JSON line: the stats, checksums of the popped S and of the popped reads, the contigs' counts, whether the host comparison held.
// Usage: test_host_bubbles reads.fa K LOWER UPPER MAX_ARM_READS ROUNDS [bad_read_cutoff]
#include "host_test.hpp"
namespace ht = elba::host_test;

int main(int argc, char **argv)
{
    return ht::run(argc, argv, 7, "reads.fa K LOWER UPPER MAX_ARM_READS ROUNDS [bad_read_cutoff]", [&] {
        const int max_arm_reads = std::atoi(argv[5]), rounds = std::atoi(argv[6]);
        const ht::Reads reads = ht::read_fasta(argv[1]);
        const ht::Front f = ht::run_to_string_graph(reads, ht::params_at(argv + 2), argc > 7 ? std::atof(argv[7]) : 0.65);
        elba::StringGraph &S = *f.S;
        const std::vector<int64_t> rows0 = S.rows, cols0 = S.cols;
        std::vector<int64_t> popped;
        const elba_bubble_stats st = elba::PopBubbles(S, reads.dna, max_arm_reads, rounds, &popped);
        const long long host_equal = S.getnnz() == st.nnz_after && (long long)rows0.size() == st.nnz_before && (long long)popped.size() == st.reads_removed &&
                                     ht::kept_in_order(rows0, cols0, popped, S);
        ht::Json j;
        j("reads", reads.size())("nnz_before", st.nnz_before)("nnz_after", st.nnz_after)("anchors", st.anchors)("arms", st.arms)
            ("bubbles", st.bubbles)("arms_removed", st.arms_removed)("reads_removed", st.reads_removed)
            ("entries_removed", st.entries_removed)("rounds_run", st.rounds_run)("s_checksum", ht::s_checksum(S))("read_checksum", ht::read_checksum(popped))
            ("host_equal", host_equal);
        ht::contig_counts(j, S, reads.dna);
        j.print();
        return 0;
    });
}
