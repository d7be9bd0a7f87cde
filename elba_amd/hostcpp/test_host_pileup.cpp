// test_host_pileup.cpp — reads -> A -> B -> PairwiseAlignment -> GetReadPileup -> PruneFull -> TransitiveReduction written against
// elba_host.hpp; every read's per-base pileup is rebuilt from its segments and GetTrimmedInterval is recomputed on it on the host.
// Prints one JSON line: counts, a checksum of the per-base pileups, and whether the host trim equals the device's on every read.
// Usage: test_host_pileup reads.fa K LOWER UPPER MODE MARGIN MIN_DEPTH MIN_RUN TRIM_LEN MASK
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include "elba_host.hpp"

int main(int argc, char **argv)
{
    if (argc < 11) { std::fprintf(stderr, "usage: %s reads.fa K LOWER UPPER MODE MARGIN MIN_DEPTH MIN_RUN TRIM_LEN MASK\n", argv[0]); return 2; }
    elba::Params prm;
    prm.kmer_size = std::atoi(argv[2]); prm.lower_kmer_freq = std::atoi(argv[3]); prm.upper_kmer_freq = std::atoi(argv[4]);
    elba_pileup_cfg cfg{};
    cfg.mode = std::atoi(argv[5]); cfg.margin = std::atoi(argv[6]); cfg.min_depth = std::atoi(argv[7]); cfg.min_run = std::atoi(argv[8]); cfg.trim_len = std::atoi(argv[9]);
    const int mask = std::atoi(argv[10]);
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
        elba_pileup_stats st{};
        std::vector<elba::PileupVector> pv = elba::GetReadPileup(mydna, *R, cfg, &st);
        unsigned long long checksum = 0, base = 0;
        long long trim_equal = 1, flagged = 0;
        for (size_t v = 0; v < pv.size(); ++v) {
            const std::vector<int> p = pv[v].pileup();
            for (size_t i = 0; i < p.size(); ++i) checksum += (unsigned long long)p[i] * ((base + i) % 1000003ull + 1);
            base += p.size();
            if (pv[v].GetTrimmedInterval(cfg.min_depth, cfg.trim_len) != pv[v].trimmed) trim_equal = 0;
            flagged += (pv[v].flags & mask) != 0;
        }
        const int64_t kept = elba::PruneFull(*R, mask);
        auto S = elba::TransitiveReduction(mydna, *R, 0.65);
        std::printf("{\"reads\": %zu, \"pairs\": %lld, \"segments\": %lld, \"pileup_checksum\": %llu, \"trim_equal\": %lld, \"flagged\": %lld, \"kept\": %lld, \"string_nnz\": %lld}\n",
                    mydna.size(), (long long)st.pairs, (long long)st.segments, checksum, trim_equal, flagged, (long long)kept, (long long)S->getnnz());
    } catch (const elba::Error &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return e.status == ELBA_ERR_NO_DEVICE ? 3 : 1;
    }
    return 0;
}
