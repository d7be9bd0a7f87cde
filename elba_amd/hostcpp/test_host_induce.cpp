// test_host_induce.cpp — a whole input assembled part by part through the C++ mirror: reads + a pair list -> elba_set_overlaps ->
// partition_components of the overlaps graph -> for every part induce_part, load_part into a second engine and
// elba_transitive_reduction there.  The pair list is text, one pair per line, ascending in (row, col), fifteen fields (host_test.hpp).
// OUT receives per part one line `part reads pairs split_pairs split_passed nnz`, one line per read of the part
// (old_of_new outside_aligned outside_passed flags) and one line per entry of the part's S (row col suffix direction, ids of the whole
// input).  Prints one JSON line of counts.
// Usage: test_host_induce reads.fa pairs.txt NPARTS out.txt [fuzz]
#include "host_test.hpp"
namespace ht = elba::host_test;

int main(int argc, char **argv)
{
    return ht::run(argc, argv, 5, "reads.fa pairs.txt NPARTS out.txt [fuzz]", [&] {
        const int nparts = std::atoi(argv[3]), fuzz = argc > 5 ? std::atoi(argv[5]) : 0;
        const ht::Reads reads = ht::read_fasta(argv[1]);
        const ht::Triples e = ht::load_pairs(argv[2]);
        elba_cfg cfg{};
        cfg.k = 17; cfg.lower = 2; cfg.upper = 8;
        elba::StringGraph W;                                     // the whole input: reads and pairs, no S needed for its overlaps graph
        W.numreads = (int64_t)reads.size();
        W.engine = std::make_shared<elba::detail::Engine>(cfg);
        elba::detail::Engine second(cfg);
        W.engine->check(elba_set_reads(W.engine->ctx, reads.dna.data(), reads.dna.offsets(), reads.dna.lengths(), W.numreads, 0));
        W.engine->check(elba_set_overlaps(W.engine->ctx, W.numreads, e.rows.data(), e.cols.data(), e.vals.data(), (int64_t)e.rows.size()));
        const elba::Partition p = elba::partition_components(W, nparts, ELBA_CC_OVERLAPS, 0, 1);
        std::ofstream out(argv[4]);
        long long sum_reads = 0, sum_pairs = 0, split = 0, split_passed = 0, nnz = 0, bad = 0, bases = 0;
        for (int part = 0; part < nparts; ++part) {
            const elba::InducedPart ip = elba::induce_part(*W.engine, p.part_of_read, part);
            elba::load_part(second, ip);
            elba_string_stats st{};
            second.check(elba_transitive_reduction(second.ctx, 0.65, fuzz, &st));
            const int64_t R = ip.numreads();
            std::vector<uint8_t> flags((size_t)(R ? R : 1));
            second.check(elba_export_read_flags(second.ctx, flags.data(), R));
            elba_overlaps_t o;
            second.check(elba_export_string_graph(second.ctx, &o));
            out << part << " " << R << " " << ip.rows.size() << " " << ip.stats.split_pairs << " " << ip.stats.split_passed << " " << o.n << "\n";
            for (int64_t w = 0; w < R; ++w)
                out << ip.old_of_new[(size_t)w] << " " << ip.outside_aligned[(size_t)w] << " " << ip.outside_passed[(size_t)w] << " " << (int)flags[(size_t)w] << "\n";
            for (int64_t a = 0; a < o.n; ++a)
                out << ip.old_of_new[(size_t)o.rows[a]] << " " << ip.old_of_new[(size_t)o.cols[a]] << " " << o.vals[a].suffix << " " << (int)o.vals[a].direction << "\n";
            sum_reads += R; sum_pairs += (long long)ip.rows.size(); split += ip.stats.split_pairs; split_passed += ip.stats.split_passed; nnz += o.n;
            bad += st.bad_reads; bases += ip.stats.bases;
            elba_free_overlaps(&o);
        }
        ht::Json()("reads", reads.size())("parts", nparts)("part_reads", sum_reads)("part_pairs", sum_pairs)("split_pairs", split)("split_passed", split_passed)
            ("string_nnz", nnz)("bad_reads", bad)("bases", bases).print();
        return 0;
    });
}
