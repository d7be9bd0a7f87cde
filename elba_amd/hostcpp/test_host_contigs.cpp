// test_host_contigs.cpp — src/main.cpp:191-332 on one rank written against elba_host.hpp, through to the contigs: reads -> A -> B ->
// PairwiseAlignment -> TransitiveReduction -> GenerateContigs -> parallel_write_contigs.  Prints one JSON line of counts.
// Usage: test_host_contigs reads.fa K LOWER UPPER out.contigs.fa [bad_read_cutoff]
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include "elba_host.hpp"

int main(int argc, char **argv)
{
    if (argc < 6) { std::fprintf(stderr, "usage: %s reads.fa K LOWER UPPER out.contigs.fa [bad_read_cutoff]\n", argv[0]); return 2; }
    elba::Params prm;
    prm.kmer_size = std::atoi(argv[2]); prm.lower_kmer_freq = std::atoi(argv[3]); prm.upper_kmer_freq = std::atoi(argv[4]);
    const double cutoff = argc > 6 ? std::atof(argv[6]) : 0.65;                             // main.cpp:61
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
        std::vector<std::string> contigs = elba::GenerateContigs(*S, mydna, &st);           // main.cpp:325
        elba::parallel_write_contigs(contigs, argv[5]);                                     // main.cpp:330
        size_t bases = 0;
        for (auto &c : contigs) bases += c.size();
        std::printf("{\"reads\": %zu, \"string_nnz\": %lld, \"contigs\": %zu, \"bases\": %zu, \"cycles\": %lld, \"branches\": %lld}\n", mydna.size(), (long long)S->getnnz(),
                    contigs.size(), bases, (long long)st.cycles, (long long)st.branches);
    } catch (const elba::Error &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return e.status == ELBA_ERR_NO_DEVICE ? 3 : 1;
    }
    return 0;
}
