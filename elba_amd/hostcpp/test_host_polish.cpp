// test_host_polish.cpp — contig polishing through the C++ mirror: reads + a pair list -> elba_set_overlaps -> elba_transitive_reduction ->
// GenerateContigs(flags) -> polish_contigs with the votes.  The pair list is text, one pair per line, ascending in (row, col):
//   row col begQ endQ begT endT rc score passed containedQ containedT direction directionT suffix suffixT
// OUT receives one line per polished contig (voters substituted deleted inserted sequence), one line per read (dist n end_j status), then
// the column counts (five per line) and the gap counts (four per line).  Prints one JSON line of counts.
// Usage: test_host_polish reads.fa pairs.txt FLAGS SKIP BAND MAX_DIFF MIN_DEPTH out.txt
#include "host_test.hpp"
namespace ht = elba::host_test;

int main(int argc, char **argv)
{
    return ht::run(argc, argv, 9, "reads.fa pairs.txt FLAGS SKIP BAND MAX_DIFF MIN_DEPTH out.txt", [&] {
        const int flags = std::atoi(argv[3]), skip = std::atoi(argv[4]), band = std::atoi(argv[5]), min_depth = std::atoi(argv[7]);
        const double max_diff = std::atof(argv[6]);
        const ht::Reads reads = ht::read_fasta(argv[1]);
        const ht::Triples pairs = ht::load_pairs(argv[2]);
        elba::StringGraph S = ht::loaded_graph(reads, pairs.rows, pairs.cols, pairs.vals, 0);
        elba_contig_stats cst{};
        std::vector<uint8_t> kinds;
        std::vector<std::string> contigs = elba::GenerateContigs(S, reads.dna, &cst, flags, &kinds);
        elba_polish_stats st{};
        const elba::Polished p = elba::polish_contigs(S, skip, band, max_diff, min_depth, true, &st);
        std::ofstream of(argv[8]);
        for (size_t k = 0; k < p.contigs.size(); ++k) of << p.voters[k] << " " << p.substituted[k] << " " << p.deleted[k] << " " << p.inserted[k] << " " << p.contigs[k] << "\n";
        for (const elba_polish_read_t &x : p.reads) of << x.dist << " " << x.n << " " << x.end_j << " " << x.status << "\n";
        for (size_t i = 0; i + 4 < p.col.size() + 1; i += 5) of << p.col[i] << " " << p.col[i + 1] << " " << p.col[i + 2] << " " << p.col[i + 3] << " " << p.col[i + 4] << "\n";
        for (size_t i = 0; i + 3 < p.gap.size() + 1; i += 4) of << p.gap[i] << " " << p.gap[i + 1] << " " << p.gap[i + 2] << " " << p.gap[i + 3] << "\n";
        ht::Json()("nreads", st.nreads)("voted", st.voted)("rejected", st.rejected)("outside", st.outside)("low_depth_columns", st.low_depth_columns)
            ("bases_before", st.bases_before)("bases_after", st.bases_after)("sum_dist", st.sum_dist)("cells", st.cells)("contigs", contigs.size()).print();
        return 0;
    });
}
