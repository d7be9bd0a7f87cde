// test_host_weak.cpp — reads -> A -> B -> PairwiseAlignment -> TransitiveReduction -> CutWeakOverlaps -> GenerateContigs, written against
// elba_host.hpp; the host copy of the cut S is held against the uncut one on the host: the rule of include/elba_amd.h is applied to the uncut
// entries with loops over columns, and the cut S must be exactly the entries it keeps, in order.
// Prints one JSON line: the stats, a checksum of the cut S, the contigs' counts, whether the host comparison held.
// Usage: test_host_weak reads.fa K LOWER UPPER MIN_RATIO_Q16 [bad_read_cutoff]
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <map>
#include "elba_host.hpp"

int main(int argc, char **argv)
{
    if (argc < 6) { std::fprintf(stderr, "usage: %s reads.fa K LOWER UPPER MIN_RATIO_Q16 [bad_read_cutoff]\n", argv[0]); return 2; }
    elba::Params prm;
    prm.kmer_size = std::atoi(argv[2]); prm.lower_kmer_freq = std::atoi(argv[3]); prm.upper_kmer_freq = std::atoi(argv[4]);
    const int q16 = std::atoi(argv[5]);
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
        std::vector<int> score0, side0;
        for (auto &o : S->vals) { score0.push_back((int)o.score); side0.push_back((int)o.direction & 1); }
        const elba_weak_stats st = elba::CutWeakOverlaps(*S, mydna, q16);
        // the rule on the uncut entries: cnt and best per (column, side), weak per entry, the mirror image by its (row, column)
        std::map<std::pair<int64_t, int>, std::pair<long long, long long>> table;      // (c, side) -> (cnt, best)
        std::map<std::pair<int64_t, int64_t>, size_t> at_of;                           // (row, col) -> entry
        for (size_t a = 0; a < rows0.size(); ++a) {
            auto it = table.find({cols0[a], side0[a]});
            if (it == table.end()) table[{cols0[a], side0[a]}] = {1, score0[a]};
            else { ++it->second.first; if (score0[a] > it->second.second) it->second.second = score0[a]; }
            at_of[{rows0[a], cols0[a]}] = a;
        }
        std::vector<char> weak(rows0.size(), 0);
        long long nweak = 0;
        for (size_t a = 0; a < rows0.size(); ++a) {
            const auto &t = table[{cols0[a], side0[a]}];
            weak[a] = t.first >= 2 && t.second > 0 && (long long)score0[a] * 65536 < (long long)q16 * t.second;
            nweak += weak[a];
        }
        long long host_equal = S->getnnz() == st.nnz_after && (long long)rows0.size() == st.nnz_before && nweak == st.weak_entries;
        size_t at = 0;
        for (size_t a = 0; a < rows0.size() && host_equal; ++a) {
            auto m = at_of.find({cols0[a], rows0[a]});
            if (weak[a] || (m != at_of.end() && weak[m->second])) continue;
            if (at >= S->rows.size() || S->rows[at] != rows0[a] || S->cols[at] != cols0[a] || (int)S->vals[at].score != score0[a]) host_equal = 0;
            ++at;
        }
        if (at != S->rows.size()) host_equal = 0;
        unsigned long long s_checksum = 0;
        for (size_t a = 0; a < S->rows.size(); ++a)
            s_checksum += (unsigned long long)(S->rows[a] + 1) * 1000003ull + (unsigned long long)S->cols[a] * 10007ull + (unsigned long long)(unsigned)S->vals[a].suffix;
        elba_contig_stats cs{};
        const std::vector<std::string> contigs = elba::GenerateContigs(*S, mydna, &cs);
        size_t bases = 0;
        for (auto &c : contigs) bases += c.size();
        std::printf("{\"reads\": %zu, \"nnz_before\": %lld, \"nnz_after\": %lld, \"branch_sides\": %lld, \"weak_entries\": %lld, \"entries_removed\": %lld, "
                    "\"sides_emptied\": %lld, \"s_checksum\": %llu, \"host_equal\": %lld, \"contigs\": %zu, \"bases\": %zu, \"branches\": %lld}\n",
                    mydna.size(), (long long)st.nnz_before, (long long)st.nnz_after, (long long)st.branch_sides, (long long)st.weak_entries,
                    (long long)st.entries_removed, (long long)st.sides_emptied, s_checksum, host_equal, contigs.size(), bases, (long long)cs.branches);
    } catch (const elba::Error &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return e.status == ELBA_ERR_NO_DEVICE ? 3 : 1;
    }
    return 0;
}
