// test_host_contigs_ex.cpp — test_host_contigs with the two extensions of the contig stage: reads -> A -> B -> PairwiseAlignment ->
// TransitiveReduction -> GenerateContigs(flags, kinds) -> parallel_write_contigs(kinds).  FLAGS: 1 circular contigs, 2 single-read contigs, 3 both;
// WITH_KINDS 0 writes the plain headers.  Prints one JSON line of counts.
// Usage: test_host_contigs_ex reads.fa K LOWER UPPER out.contigs.fa FLAGS WITH_KINDS [bad_read_cutoff]
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include "elba_host.hpp"

int main(int argc, char **argv)
{
    if (argc < 8) { std::fprintf(stderr, "usage: %s reads.fa K LOWER UPPER out.contigs.fa FLAGS WITH_KINDS [bad_read_cutoff]\n", argv[0]); return 2; }
    elba::Params prm;
    prm.kmer_size = std::atoi(argv[2]); prm.lower_kmer_freq = std::atoi(argv[3]); prm.upper_kmer_freq = std::atoi(argv[4]);
    const int flags = std::atoi(argv[6]), with_kinds = std::atoi(argv[7]);
    const double cutoff = argc > 8 ? std::atof(argv[8]) : 0.65;                             // main.cpp:61
    std::ifstream in(argv[1]);
    std::vector<std::string> seqs;
    std::string line, cur;
    while (std::getline(in, line)) {
        if (!line.empty() && line[0] == '>') { if (!cur.empty()) seqs.push_back(cur); cur.clear(); }
        else cur += line;
    }
    if (!cur.empty()) seqs.push_back(cur);
    std::vector<size_t> lens;
    for (auto &s : seqs) lens.push_back(s.size());
    elba::DnaBuffer mydna(elba::DnaBuffer::computebufsize(lens));
    for (auto &s : seqs) mydna.push_back(s.c_str(), s.size());
    auto commgrid = std::make_shared<elba::Grid>();
    try {
        auto kmermap = elba::get_kmer_count_map_keys(mydna, commgrid, prm);                // main.cpp:192
        elba::get_kmer_count_map_values(mydna, *kmermap, commgrid);                         // main.cpp:225
        auto A = elba::create_kmer_matrix(mydna, *kmermap, commgrid);                       // main.cpp:259
        kmermap.reset();
        auto AT = std::make_unique<elba::KmerMatrix>(*A);                                   // main.cpp:272-273
        AT->Transpose();
        auto B = elba::create_seed_matrix(*A, *AT);                                         // main.cpp:281
        A.reset(); AT.reset();
        auto R = elba::PairwiseAlignment(mydna, *B, 1, -1, -1, 15);                         // main.cpp:300
        auto S = elba::TransitiveReduction(mydna, *R, cutoff);                              // main.cpp:305-312
        elba_contig_stats st{};
        std::vector<uint8_t> kinds;
        std::vector<std::string> contigs = elba::GenerateContigs(*S, mydna, &st, flags, &kinds);
        elba::parallel_write_contigs(contigs, argv[5], with_kinds ? &kinds : nullptr);
        size_t bases = 0, circular = 0, single = 0;
        for (auto &c : contigs) bases += c.size();
        for (uint8_t k : kinds) { circular += k == 1; single += k == 2; }
        std::printf("{\"reads\": %zu, \"string_nnz\": %lld, \"contigs\": %zu, \"bases\": %zu, \"cycles\": %lld, \"branches\": %lld, \"circular\": %zu, \"single\": %zu}\n",
                    mydna.size(), (long long)S->getnnz(), contigs.size(), bases, (long long)st.cycles, (long long)st.branches, circular, single);
    } catch (const elba::Error &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return e.status == ELBA_ERR_NO_DEVICE ? 3 : 1;
    }
    return 0;
}
