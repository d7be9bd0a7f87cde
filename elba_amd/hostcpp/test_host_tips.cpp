// test_host_tips.cpp — reads -> A -> B -> PairwiseAlignment -> TransitiveReduction -> ClipTips -> GenerateContigs, written against
// elba_host.hpp; the host copy of the clipped S is held against the unclipped one on the host: it must be its entries without those of
// the clipped reads, in order.
// Prints one JSON line: the stats, checksums of the clipped S and of the clipped reads, the contigs' counts, whether the host comparison held.
// Usage: test_host_tips reads.fa K LOWER UPPER MAX_TIP_READS ROUNDS [bad_read_cutoff]
#include "host_test.hpp"
namespace ht = elba::host_test;

int main(int argc, char **argv)
{
    return ht::run(argc, argv, 7, "reads.fa K LOWER UPPER MAX_TIP_READS ROUNDS [bad_read_cutoff]", [&] {
        const int max_tip_reads = std::atoi(argv[5]), rounds = std::atoi(argv[6]);
        const ht::Reads reads = ht::read_fasta(argv[1]);
        const ht::Front f = ht::run_to_string_graph(reads, ht::params_at(argv + 2), argc > 7 ? std::atof(argv[7]) : 0.65);
        elba::StringGraph &S = *f.S;
        const std::vector<int64_t> rows0 = S.rows, cols0 = S.cols;
        std::vector<int64_t> clipped;
        const elba_tip_stats st = elba::ClipTips(S, reads.dna, max_tip_reads, rounds, &clipped);
        const long long host_equal = S.getnnz() == st.nnz_after && (long long)rows0.size() == st.nnz_before && (long long)clipped.size() == st.reads_removed &&
                                     ht::kept_in_order(rows0, cols0, clipped, S);
        ht::Json j;
        j("reads", reads.size())("nnz_before", st.nnz_before)("nnz_after", st.nnz_after)("dead_ends", st.dead_ends)("tips", st.tips)
            ("reads_removed", st.reads_removed)("entries_removed", st.entries_removed)("spared_anchors", st.spared_anchors)
            ("rounds_run", st.rounds_run)("s_checksum", ht::s_checksum(S))("read_checksum", ht::read_checksum(clipped))("host_equal", host_equal);
        ht::contig_counts(j, S, reads.dna);
        j.print();
        return 0;
    });
}
