// test_host_components.cpp — connected components through the C++ mirror: reads + an edge list -> elba_set_overlaps ->
// elba_transitive_reduction -> graph_components of both graphs -> partition_components.  The edge list is text, one pair per line,
// ascending in (row, col):
//   row col direction directionT suffix suffixT
// OUT receives one line per read (component in S, component among the overlaps, part), then one line per component of S
// (first_read reads bases edges branches ends), then the part weights on one line.  Prints one JSON line of counts.
// Usage: test_host_components reads.fa edges.txt NPARTS out.txt [fuzz]
#include "host_test.hpp"
namespace ht = elba::host_test;

int main(int argc, char **argv)
{
    return ht::run(argc, argv, 5, "reads.fa edges.txt NPARTS out.txt [fuzz]", [&] {
        const int nparts = std::atoi(argv[3]), fuzz = argc > 5 ? std::atoi(argv[5]) : 0;
        const ht::Reads reads = ht::read_fasta(argv[1]);
        const ht::Triples e = ht::load_edges(argv[2]);
        elba::StringGraph S = ht::loaded_graph(reads, e.rows, e.cols, e.vals, fuzz);
        elba_cc_stats st{}, sto{};
        const elba::Components cs = elba::graph_components(S, ELBA_CC_STRING, true, &st);
        const elba::Components co = elba::graph_components(S, ELBA_CC_OVERLAPS, false, &sto);
        const elba::Partition p = elba::partition_components(S, nparts, ELBA_CC_STRING, 1, 2);
        std::ofstream out(argv[4]);
        for (size_t v = 0; v < cs.comp_of_read.size(); ++v) out << cs.comp_of_read[v] << " " << co.comp_of_read[v] << " " << p.part_of_read[v] << "\n";
        for (size_t c = 0; c < cs.reads.size(); ++c)
            out << cs.first_read[c] << " " << cs.reads[c] << " " << cs.bases[c] << " " << cs.edges[c] << " " << cs.branches[c] << " " << cs.ends[c] << "\n";
        for (size_t q = 0; q < p.part_weight.size(); ++q) out << p.part_weight[q] << (q + 1 < p.part_weight.size() ? " " : "\n");
        ht::Json()("reads", reads.size())("string_nnz", S.stats.nnz)("components", st.components)("used_components", st.used_components)("isolated", st.isolated)
            ("largest_reads", st.largest_reads)("largest_bases", st.largest_bases)("edges", st.edges)("overlap_components", sto.components)("overlap_edges", sto.edges).print();
        return 0;
    });
}
