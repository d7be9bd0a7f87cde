// test_host_bridges.cpp — reads -> A -> B -> PairwiseAlignment -> TransitiveReduction -> CutBridges -> GenerateContigs, written against
// elba_host.hpp; the host copy of the cut S is held against the uncut one on the host: it must be its entries without those of
// the bridge reads, in order.
// Prints one JSON line: the stats, checksums of the cut S and of the bridge reads, the contigs' counts, whether the host comparison held.
// Usage: test_host_bridges reads.fa K LOWER UPPER MAX_BRIDGE_READS MIN_FLANK_READS [bad_read_cutoff]
#include "host_test.hpp"
namespace ht = elba::host_test;

int main(int argc, char **argv)
{
    return ht::run(argc, argv, 7, "reads.fa K LOWER UPPER MAX_BRIDGE_READS MIN_FLANK_READS [bad_read_cutoff]", [&] {
        const int max_bridge_reads = std::atoi(argv[5]), min_flank_reads = std::atoi(argv[6]);
        const ht::Reads reads = ht::read_fasta(argv[1]);
        const ht::Front f = ht::run_to_string_graph(reads, ht::params_at(argv + 2), argc > 7 ? std::atof(argv[7]) : 0.65);
        elba::StringGraph &S = *f.S;
        const std::vector<int64_t> rows0 = S.rows, cols0 = S.cols;
        std::vector<int64_t> cut;
        const elba_bridge_stats st = elba::CutBridges(S, reads.dna, max_bridge_reads, min_flank_reads, &cut);
        const long long host_equal = S.getnnz() == st.nnz_after && (long long)rows0.size() == st.nnz_before && (long long)cut.size() == st.reads_removed &&
                                     ht::kept_in_order(rows0, cols0, cut, S);
        ht::Json j;
        j("reads", reads.size())("nnz_before", st.nnz_before)("nnz_after", st.nnz_after)("anchors", st.anchors)("chains", st.chains)
            ("long_flanks", st.long_flanks)("bridges", st.bridges)("reads_removed", st.reads_removed)
            ("entries_removed", st.entries_removed)("s_checksum", ht::s_checksum(S))("read_checksum", ht::read_checksum(cut))("host_equal", host_equal);
        ht::contig_counts(j, S, reads.dna);
        j.print();
        return 0;
    });
}
