// test_host_polish.cpp — contig polishing through the C++ mirror: reads + a pair list -> elba_set_overlaps -> elba_transitive_reduction ->
// GenerateContigs(flags) -> polish_contigs with the votes.  The pair list is text, one pair per line, ascending in (row, col):
//   row col begQ endQ begT endT rc score passed containedQ containedT direction directionT suffix suffixT
// OUT receives one line per polished contig (voters substituted deleted inserted sequence), one line per read (dist n end_j status), then
// the column counts (five per line) and the gap counts (four per line).  Prints one JSON line of counts.
// Usage: test_host_polish reads.fa pairs.txt FLAGS SKIP BAND MAX_DIFF MIN_DEPTH out.txt
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include "elba_host.hpp"

int main(int argc, char **argv)
{
    if (argc < 9) { std::fprintf(stderr, "usage: %s reads.fa pairs.txt FLAGS SKIP BAND MAX_DIFF MIN_DEPTH out.txt\n", argv[0]); return 2; }
    const int flags = std::atoi(argv[3]), skip = std::atoi(argv[4]), band = std::atoi(argv[5]), min_depth = std::atoi(argv[7]);
    const double max_diff = std::atof(argv[6]);
    std::ifstream in(argv[1]);
    std::vector<std::string> seqs;
    std::string line, cur;
    bool open = false;
    while (std::getline(in, line)) {
        if (!line.empty() && line[0] == '>') { if (open) seqs.push_back(cur); cur.clear(); open = true; }
        else cur += line;
    }
    if (open) seqs.push_back(cur);
    std::vector<size_t> lens;
    for (auto &s : seqs) lens.push_back(s.size());
    elba::DnaBuffer mydna(elba::DnaBuffer::computebufsize(lens));
    for (auto &s : seqs) mydna.push_back(s.c_str(), s.size());
    std::vector<int64_t> rows, cols;
    std::vector<elba_overlap_t> vals;
    std::ifstream pin(argv[2]);
    long long r, c, v[13];
    while (pin >> r >> c) {
        for (long long &x : v) pin >> x;
        elba_overlap_t o{};
        o.begQ = (int32_t)v[0]; o.endQ = (int32_t)v[1]; o.begT = (int32_t)v[2]; o.endT = (int32_t)v[3]; o.rc = (uint8_t)v[4]; o.score = (int32_t)v[5]; o.passed = (uint8_t)v[6];
        o.containedQ = (uint8_t)v[7]; o.containedT = (uint8_t)v[8]; o.direction = (int8_t)v[9]; o.directionT = (int8_t)v[10]; o.suffix = (int32_t)v[11]; o.suffixT = (int32_t)v[12];
        rows.push_back(r); cols.push_back(c); vals.push_back(o);
    }
    try {
        elba_cfg cfg{};
        cfg.k = 17; cfg.lower = 2; cfg.upper = 8;
        elba::StringGraph S;
        S.numreads = (int64_t)mydna.size();
        S.engine = std::make_shared<elba::detail::Engine>(cfg);
        elba_ctx *ctx = S.engine->ctx;
        S.engine->check(elba_set_reads(ctx, mydna.data(), mydna.offsets(), mydna.lengths(), (int64_t)mydna.size(), 0));
        S.engine->check(elba_set_overlaps(ctx, S.numreads, rows.data(), cols.data(), vals.data(), (int64_t)rows.size()));
        S.engine->check(elba_transitive_reduction(ctx, 0.0, 0, &S.stats));
        elba_contig_stats cst{};
        std::vector<uint8_t> kinds;
        std::vector<std::string> contigs = elba::GenerateContigs(S, mydna, &cst, flags, &kinds);
        elba_polish_stats st{};
        const elba::Polished p = elba::polish_contigs(S, skip, band, max_diff, min_depth, true, &st);
        std::ofstream of(argv[8]);
        for (size_t k = 0; k < p.contigs.size(); ++k) of << p.voters[k] << " " << p.substituted[k] << " " << p.deleted[k] << " " << p.inserted[k] << " " << p.contigs[k] << "\n";
        for (const elba_polish_read_t &x : p.reads) of << x.dist << " " << x.n << " " << x.end_j << " " << x.status << "\n";
        for (size_t i = 0; i + 4 < p.col.size() + 1; i += 5) of << p.col[i] << " " << p.col[i + 1] << " " << p.col[i + 2] << " " << p.col[i + 3] << " " << p.col[i + 4] << "\n";
        for (size_t i = 0; i + 3 < p.gap.size() + 1; i += 4) of << p.gap[i] << " " << p.gap[i + 1] << " " << p.gap[i + 2] << " " << p.gap[i + 3] << "\n";
        std::printf("{\"nreads\": %lld, \"voted\": %lld, \"rejected\": %lld, \"outside\": %lld, \"low_depth_columns\": %lld, \"bases_before\": %lld, \"bases_after\": %lld, "
                    "\"sum_dist\": %lld, \"cells\": %lld, \"contigs\": %zu}\n",
                    (long long)st.nreads, (long long)st.voted, (long long)st.rejected, (long long)st.outside, (long long)st.low_depth_columns, (long long)st.bases_before,
                    (long long)st.bases_after, (long long)st.sum_dist, (long long)st.cells, contigs.size());
    } catch (const elba::Error &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return e.status == ELBA_ERR_NO_DEVICE ? 3 : 1;
    }
    return 0;
}
