// test_host_place.cpp — read placements through the C++ mirror: reads + a pair list -> elba_set_overlaps -> elba_transitive_reduction ->
// GenerateContigs(flags, kinds) -> place_reads -> write_placements_paf + write_gfa with the depth tag.  The pair list is text, one pair per
// line, ascending in (row, col):
//   row col begQ endQ begT endT rc score passed containedQ containedT direction directionT suffix suffixT
// RECORDS receives one line per read (start contig anchor score strand kind flags), then one line per contig (segments, credited reads,
// credited bases) followed by its segments (start depth).  Prints one JSON line of counts.
// Usage: test_host_place reads.fa pairs.txt FLAGS SKIP out.paf out.gfa out.records
#include "host_test.hpp"
namespace ht = elba::host_test;

int main(int argc, char **argv)
{
    return ht::run(argc, argv, 8, "reads.fa pairs.txt FLAGS SKIP out.paf out.gfa out.records", [&] {
        const int flags = std::atoi(argv[3]), skip = std::atoi(argv[4]);
        const ht::Reads reads = ht::read_fasta(argv[1]);
        const ht::Triples pairs = ht::load_pairs(argv[2]);
        elba::StringGraph S = ht::loaded_graph(reads, pairs.rows, pairs.cols, pairs.vals, 0);
        elba_contig_stats cst{};
        std::vector<uint8_t> kinds;
        std::vector<std::string> contigs = elba::GenerateContigs(S, reads.dna, &cst, flags, &kinds);
        elba_place_stats st{};
        const elba::Placements pl = elba::place_reads(S, skip, &st);
        std::vector<int64_t> lens64, contig_lens;
        for (auto &s : reads.seqs) lens64.push_back((int64_t)s.size());
        for (auto &s : contigs) contig_lens.push_back((int64_t)s.size());
        elba::write_placements_paf(argv[5], pl, reads.names, lens64, contig_lens, &kinds);
        elba::write_gfa(argv[6], contigs, &kinds, elba::assembly_links(S), nullptr, &pl.credited_bases);
        std::ofstream rf(argv[7]);
        for (const elba_placement_t &p : pl.reads)
            rf << p.start << " " << p.contig << " " << p.anchor << " " << p.score << " " << (int)p.strand << " " << (int)p.kind << " " << (int)p.flags << "\n";
        for (size_t k = 0; k < contigs.size(); ++k) {
            rf << pl.seg_off[k + 1] - pl.seg_off[k] << " " << pl.credited_reads[k] << " " << pl.credited_bases[k] << "\n";
            for (int64_t j = pl.seg_off[k]; j < pl.seg_off[k + 1]; ++j) rf << pl.seg_start[(size_t)j] << " " << pl.seg_depth[(size_t)j] << "\n";
        }
        ht::Json()("nreads", st.nreads)("chain", st.chain)("anchored", st.anchored)("unanchored", st.unanchored)("skipped", st.skipped)("empty", st.empty)
            ("candidates", st.candidates)("clipped", st.clipped)("outside", st.outside)("wrapped", st.wrapped)("segments", st.segments)("max_depth", st.max_depth)
            ("credited_bases", st.credited_bases)("contigs", contigs.size()).print();
        return 0;
    });
}
