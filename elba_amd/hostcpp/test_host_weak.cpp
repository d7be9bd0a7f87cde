// test_host_weak.cpp — reads -> A -> B -> PairwiseAlignment -> TransitiveReduction -> CutWeakOverlaps -> GenerateContigs, written against
// elba_host.hpp; the host copy of the cut S is held against the uncut one on the host: the rule of include/elba_amd.h is applied to the uncut
// entries with loops over columns, and the cut S must be exactly the entries it keeps, in order.
// Prints one JSON line: the stats, a checksum of the cut S, the contigs' counts, whether the host comparison held.
// Usage: test_host_weak reads.fa K LOWER UPPER MIN_RATIO_Q16 [bad_read_cutoff]
#include <map>
#include "host_test.hpp"
namespace ht = elba::host_test;

int main(int argc, char **argv)
{
    return ht::run(argc, argv, 6, "reads.fa K LOWER UPPER MIN_RATIO_Q16 [bad_read_cutoff]", [&] {
        const int q16 = std::atoi(argv[5]);
        const ht::Reads reads = ht::read_fasta(argv[1]);
        const ht::Front f = ht::run_to_string_graph(reads, ht::params_at(argv + 2), argc > 6 ? std::atof(argv[6]) : 0.65);
        elba::StringGraph &S = *f.S;
        const std::vector<int64_t> rows0 = S.rows, cols0 = S.cols;
        std::vector<int> score0, side0;
        for (auto &o : S.vals) { score0.push_back((int)o.score); side0.push_back((int)o.direction & 1); }
        const elba_weak_stats st = elba::CutWeakOverlaps(S, reads.dna, q16);
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
        long long host_equal = S.getnnz() == st.nnz_after && (long long)rows0.size() == st.nnz_before && nweak == st.weak_entries;
        size_t at = 0;
        for (size_t a = 0; a < rows0.size() && host_equal; ++a) {
            auto m = at_of.find({cols0[a], rows0[a]});
            if (weak[a] || (m != at_of.end() && weak[m->second])) continue;
            if (at >= S.rows.size() || S.rows[at] != rows0[a] || S.cols[at] != cols0[a] || (int)S.vals[at].score != score0[a]) host_equal = 0;
            ++at;
        }
        if (at != S.rows.size()) host_equal = 0;
        ht::Json j;
        j("reads", reads.size())("nnz_before", st.nnz_before)("nnz_after", st.nnz_after)("branch_sides", st.branch_sides)
            ("weak_entries", st.weak_entries)("entries_removed", st.entries_removed)("sides_emptied", st.sides_emptied)
            ("s_checksum", ht::s_checksum(S))("host_equal", host_equal);
        ht::contig_counts(j, S, reads.dna);
        j.print();
        return 0;
    });
}
