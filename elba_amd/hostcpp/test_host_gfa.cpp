// test_host_gfa.cpp — the assembly graph through the C++ mirror: reads + an edge list -> elba_set_overlaps -> elba_transitive_reduction ->
// GenerateContigs(flags, kinds) -> assembly_links -> write_gfa.  The edge list is text, one pair per line, ascending in (row, col):
//   row col direction directionT suffix suffixT
// LINKS receives one record per line (from to from_read to_read overlap from_rev to_rev flags).  Prints one JSON line of counts.
// Usage: test_host_gfa reads.fa edges.txt FLAGS out.gfa out.links [fuzz]
#include "host_test.hpp"
namespace ht = elba::host_test;

int main(int argc, char **argv)
{
    return ht::run(argc, argv, 6, "reads.fa edges.txt FLAGS out.gfa out.links [fuzz]", [&] {
        const int flags = std::atoi(argv[3]), fuzz = argc > 6 ? std::atoi(argv[6]) : 0;
        const ht::Reads reads = ht::read_fasta(argv[1]);
        const ht::Triples e = ht::load_edges(argv[2]);
        elba::StringGraph S = ht::loaded_graph(reads, e.rows, e.cols, e.vals, fuzz);
        elba_contig_stats cst{};
        std::vector<uint8_t> kinds;
        std::vector<std::string> contigs = elba::GenerateContigs(S, reads.dna, &cst, flags, &kinds);
        elba_graph_stats st{};
        std::vector<elba_link_t> links = elba::assembly_links(S, &st);
        elba_contigs_t ec;
        S.engine->check(elba_export_contigs(S.engine->ctx, &ec));
        std::vector<int64_t> chain_reads;
        for (int64_t i = 0; i < ec.n; ++i) chain_reads.push_back(ec.chain_off[i + 1] - ec.chain_off[i]);
        elba_free_contigs(&ec);
        elba::write_gfa(argv[4], contigs, &kinds, links, &chain_reads);
        std::ofstream lf(argv[5]);
        for (const elba_link_t &l : links)
            lf << l.from << " " << l.to << " " << l.from_read << " " << l.to_read << " " << l.overlap << " " << (int)l.from_rev << " " << (int)l.to_rev << " " << (int)l.flags << "\n";
        ht::Json()("reads", reads.size())("string_nnz", S.stats.nnz)("records", links.size())("segments", st.segments)("candidates", st.candidates)("links", st.links)
            ("closures", st.closures)("twisted", st.twisted)("unplaced", st.unplaced)("clamped", st.clamped)("asymmetric", st.asymmetric).print();
        return 0;
    });
}
