// test_host_stars.cpp — reads -> A -> B -> PairwiseAlignment -> TransitiveReduction -> ResolveStars -> GenerateContigs, written against
// elba_host.hpp; the host copy of the resolved S is held against the unresolved one on the host: it must be its entries without those of
// the odd arms, in order.
// Prints one JSON line: the stats, checksums of the resolved S and of the odd arms, the contigs' counts, whether the host comparison held.
// Usage: test_host_stars reads.fa K LOWER UPPER ROUNDS [bad_read_cutoff]
#include "host_test.hpp"
namespace ht = elba::host_test;

int main(int argc, char **argv)
{
    return ht::run(argc, argv, 6, "reads.fa K LOWER UPPER ROUNDS [bad_read_cutoff]", [&] {
        const int rounds = std::atoi(argv[5]);
        const ht::Reads reads = ht::read_fasta(argv[1]);
        const ht::Front f = ht::run_to_string_graph(reads, ht::params_at(argv + 2), argc > 6 ? std::atof(argv[6]) : 0.65);
        elba::StringGraph &S = *f.S;
        const std::vector<int64_t> rows0 = S.rows, cols0 = S.cols;
        std::vector<int64_t> odd;
        const elba_star_stats st = elba::ResolveStars(S, reads.dna, rounds, &odd);
        const long long host_equal = S.getnnz() == st.nnz_after && (long long)rows0.size() == st.nnz_before && (long long)odd.size() == st.reads_removed &&
                                     ht::kept_in_order(rows0, cols0, odd, S);
        ht::Json j;
        j("reads", reads.size())("nnz_before", st.nnz_before)("nnz_after", st.nnz_after)("centres", st.centres)("pairs0", st.pairs0)
            ("pairs1", st.pairs1)("pairs2", st.pairs2)("pairs3", st.pairs3)("reads_removed", st.reads_removed)
            ("entries_removed", st.entries_removed)("rounds_run", st.rounds_run)("s_checksum", ht::s_checksum(S))("read_checksum", ht::read_checksum(odd))
            ("host_equal", host_equal);
        ht::contig_counts(j, S, reads.dna);
        j.print();
        return 0;
    });
}
