// test_host_contigs.cpp — src/main.cpp:191-332 on one rank written against elba_host.hpp, through to the contigs: reads -> A -> B ->
// PairwiseAlignment -> TransitiveReduction -> GenerateContigs -> parallel_write_contigs.  Prints one JSON line of counts.
// Usage: test_host_contigs reads.fa K LOWER UPPER out.contigs.fa [bad_read_cutoff]
#include "host_test.hpp"
namespace ht = elba::host_test;

int main(int argc, char **argv)
{
    return ht::run(argc, argv, 6, "reads.fa K LOWER UPPER out.contigs.fa [bad_read_cutoff]", [&] {
        const double cutoff = argc > 6 ? std::atof(argv[6]) : 0.65;                             // main.cpp:61
        const ht::Reads reads = ht::read_fasta(argv[1]);
        const ht::Front f = ht::run_to_string_graph(reads, ht::params_at(argv + 2), cutoff);    // main.cpp:192-312
        elba_contig_stats st{};
        std::vector<std::string> contigs = elba::GenerateContigs(*f.S, reads.dna, &st);         // main.cpp:325
        elba::parallel_write_contigs(contigs, argv[5]);                                         // main.cpp:330
        size_t bases = 0;
        for (auto &c : contigs) bases += c.size();
        ht::Json()("reads", reads.size())("string_nnz", f.S->getnnz())("contigs", contigs.size())("bases", bases)("cycles", st.cycles)("branches", st.branches).print();
        return 0;
    });
}
