// test_host_stars.cpp — reads -> A -> B -> PairwiseAlignment -> TransitiveReduction -> ResolveStars -> GenerateContigs, written against
// elba_host.hpp; the host copy of the resolved S is held against the unresolved one on the host: it must be its entries without those of
// the odd arms, in order.
// Prints one JSON line: the stats, checksums of the resolved S and of the odd arms, the contigs' counts, whether the host comparison held.
// Usage: test_host_stars reads.fa K LOWER UPPER ROUNDS [bad_read_cutoff]
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include "elba_host.hpp"

int main(int argc, char **argv)
{
    if (argc < 6) { std::fprintf(stderr, "usage: %s reads.fa K LOWER UPPER ROUNDS [bad_read_cutoff]\n", argv[0]); return 2; }
    elba::Params prm;
    prm.kmer_size = std::atoi(argv[2]); prm.lower_kmer_freq = std::atoi(argv[3]); prm.upper_kmer_freq = std::atoi(argv[4]);
    const int rounds = std::atoi(argv[5]);
    const double cutoff = argc > 6 ? std::atof(argv[6]) : 0.65;
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
        auto kmermap = elba::get_kmer_count_map_keys(mydna, commgrid, prm);
        elba::get_kmer_count_map_values(mydna, *kmermap, commgrid);
        auto A = elba::create_kmer_matrix(mydna, *kmermap, commgrid);
        kmermap.reset();
        auto AT = std::make_unique<elba::KmerMatrix>(*A);
        AT->Transpose();
        auto B = elba::create_seed_matrix(*A, *AT);
        A.reset(); AT.reset();
        auto R = elba::PairwiseAlignment(mydna, *B, 1, -1, -1, 15);
        auto S = elba::TransitiveReduction(mydna, *R, cutoff);
        const std::vector<int64_t> rows0 = S->rows, cols0 = S->cols;
        std::vector<int64_t> odd;
        const elba_star_stats st = elba::ResolveStars(*S, mydna, rounds, &odd);
        std::vector<uint8_t> gone(mydna.size(), 0);
        unsigned long long read_checksum = 0, s_checksum = 0;
        for (int64_t v : odd) { gone[(size_t)v] = 1; read_checksum += (unsigned long long)(v + 1) * 10007ull; }
        long long host_equal = S->getnnz() == st.nnz_after && (long long)rows0.size() == st.nnz_before && (long long)odd.size() == st.reads_removed;
        size_t at = 0;
        for (size_t a = 0; a < rows0.size() && host_equal; ++a) {
            if (gone[(size_t)rows0[a]] || gone[(size_t)cols0[a]]) continue;
            if (at >= S->rows.size() || S->rows[at] != rows0[a] || S->cols[at] != cols0[a]) host_equal = 0;
            ++at;
        }
        if (at != S->rows.size()) host_equal = 0;
        for (size_t a = 0; a < S->rows.size(); ++a)
            s_checksum += (unsigned long long)(S->rows[a] + 1) * 1000003ull + (unsigned long long)S->cols[a] * 10007ull + (unsigned long long)(unsigned)S->vals[a].suffix;
        elba_contig_stats cs{};
        const std::vector<std::string> contigs = elba::GenerateContigs(*S, mydna, &cs);
        size_t bases = 0;
        for (auto &c : contigs) bases += c.size();
        std::printf("{\"reads\": %zu, \"nnz_before\": %lld, \"nnz_after\": %lld, \"centres\": %lld, \"pairs0\": %lld, \"pairs1\": %lld, \"pairs2\": %lld, \"pairs3\": %lld, "
                    "\"reads_removed\": %lld, \"entries_removed\": %lld, \"rounds_run\": %d, \"s_checksum\": %llu, \"read_checksum\": %llu, \"host_equal\": %lld, "
                    "\"contigs\": %zu, \"bases\": %zu, \"branches\": %lld}\n",
                    mydna.size(), (long long)st.nnz_before, (long long)st.nnz_after, (long long)st.centres, (long long)st.pairs0, (long long)st.pairs1,
                    (long long)st.pairs2, (long long)st.pairs3, (long long)st.reads_removed, (long long)st.entries_removed, (int)st.rounds_run, s_checksum, read_checksum,
                    host_equal, contigs.size(), bases, (long long)cs.branches);
    } catch (const elba::Error &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return e.status == ELBA_ERR_NO_DEVICE ? 3 : 1;
    }
    return 0;
}
