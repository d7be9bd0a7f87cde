// test_host_contigs_ex.cpp — test_host_contigs with the two extensions of the contig stage: reads -> A -> B -> PairwiseAlignment ->
// TransitiveReduction -> GenerateContigs(flags, kinds) -> parallel_write_contigs(kinds).  FLAGS: 1 circular contigs, 2 single-read contigs, 3 both;
// WITH_KINDS 0 writes the plain headers.  Prints one JSON line of counts.
// Usage: test_host_contigs_ex reads.fa K LOWER UPPER out.contigs.fa FLAGS WITH_KINDS [bad_read_cutoff]
#include "host_test.hpp"
namespace ht = elba::host_test;

int main(int argc, char **argv)
{
    return ht::run(argc, argv, 8, "reads.fa K LOWER UPPER out.contigs.fa FLAGS WITH_KINDS [bad_read_cutoff]", [&] {
        const int flags = std::atoi(argv[6]), with_kinds = std::atoi(argv[7]);
        const double cutoff = argc > 8 ? std::atof(argv[8]) : 0.65;                             // main.cpp:61
        const ht::Reads reads = ht::read_fasta(argv[1]);
        const ht::Front f = ht::run_to_string_graph(reads, ht::params_at(argv + 2), cutoff);    // main.cpp:192-312
        elba_contig_stats st{};
        std::vector<uint8_t> kinds;
        std::vector<std::string> contigs = elba::GenerateContigs(*f.S, reads.dna, &st, flags, &kinds);
        elba::parallel_write_contigs(contigs, argv[5], with_kinds ? &kinds : nullptr);
        size_t bases = 0, circular = 0, single = 0;
        for (auto &c : contigs) bases += c.size();
        for (uint8_t k : kinds) { circular += k == 1; single += k == 2; }
        ht::Json()("reads", reads.size())("string_nnz", f.S->getnnz())("contigs", contigs.size())("bases", bases)("cycles", st.cycles)("branches", st.branches)
            ("circular", circular)("single", single).print();
        return 0;
    });
}
