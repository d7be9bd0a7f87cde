// test_host_pileup.cpp — reads -> A -> B -> PairwiseAlignment -> GetReadPileup -> PruneFull -> TransitiveReduction written against
// elba_host.hpp; every read's per-base pileup is rebuilt from its segments and GetTrimmedInterval is recomputed on it on the host.
// Prints one JSON line: counts, a checksum of the per-base pileups, and whether the host trim equals the device's on every read.
// Usage: test_host_pileup reads.fa K LOWER UPPER MODE MARGIN MIN_DEPTH MIN_RUN TRIM_LEN MASK
#include "host_test.hpp"
namespace ht = elba::host_test;

int main(int argc, char **argv)
{
    return ht::run(argc, argv, 11, "reads.fa K LOWER UPPER MODE MARGIN MIN_DEPTH MIN_RUN TRIM_LEN MASK", [&] {
        elba_pileup_cfg cfg{};
        cfg.mode = std::atoi(argv[5]); cfg.margin = std::atoi(argv[6]); cfg.min_depth = std::atoi(argv[7]); cfg.min_run = std::atoi(argv[8]); cfg.trim_len = std::atoi(argv[9]);
        const int mask = std::atoi(argv[10]);
        const ht::Reads reads = ht::read_fasta(argv[1]);
        const ht::Front f = ht::run_to_string_graph(reads, ht::params_at(argv + 2), 0.65, ht::Stop::R);
        elba_pileup_stats st{};
        std::vector<elba::PileupVector> pv = elba::GetReadPileup(reads.dna, *f.R, cfg, &st);
        unsigned long long checksum = 0, base = 0;
        long long trim_equal = 1, flagged = 0;
        for (size_t v = 0; v < pv.size(); ++v) {
            const std::vector<int> p = pv[v].pileup();
            for (size_t i = 0; i < p.size(); ++i) checksum += (unsigned long long)p[i] * ((base + i) % 1000003ull + 1);
            base += p.size();
            if (pv[v].GetTrimmedInterval(cfg.min_depth, cfg.trim_len) != pv[v].trimmed) trim_equal = 0;
            flagged += (pv[v].flags & mask) != 0;
        }
        const int64_t kept = elba::PruneFull(*f.R, mask);
        auto S = elba::TransitiveReduction(reads.dna, *f.R, 0.65);
        ht::Json()("reads", reads.size())("pairs", st.pairs)("segments", st.segments)("pileup_checksum", checksum)("trim_equal", trim_equal)("flagged", flagged)("kept", kept)
            ("string_nnz", S->getnnz()).print();
        return 0;
    });
}
