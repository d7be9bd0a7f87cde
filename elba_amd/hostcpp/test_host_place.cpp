// test_host_place.cpp — read placements through the C++ mirror: reads + a pair list -> elba_set_overlaps -> elba_transitive_reduction ->
// GenerateContigs(flags, kinds) -> place_reads -> write_placements_paf + write_gfa with the depth tag.  The pair list is text, one pair per
// line, ascending in (row, col):
//   row col begQ endQ begT endT rc score passed containedQ containedT direction directionT suffix suffixT
// RECORDS receives one line per read (start contig anchor score strand kind flags), then one line per contig (segments, credited reads,
// credited bases) followed by its segments (start depth).  Prints one JSON line of counts.
// Usage: test_host_place reads.fa pairs.txt FLAGS SKIP out.paf out.gfa out.records
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include "elba_host.hpp"

int main(int argc, char **argv)
{
    if (argc < 8) { std::fprintf(stderr, "usage: %s reads.fa pairs.txt FLAGS SKIP out.paf out.gfa out.records\n", argv[0]); return 2; }
    const int flags = std::atoi(argv[3]), skip = std::atoi(argv[4]);
    std::ifstream in(argv[1]);
    std::vector<std::string> seqs, names;
    std::string line, cur;
    bool open = false;
    while (std::getline(in, line)) {
        if (!line.empty() && line[0] == '>') { if (open) seqs.push_back(cur); cur.clear(); open = true; names.push_back(line.substr(1)); }
        else cur += line;
    }
    if (open) seqs.push_back(cur);
    std::vector<size_t> lens;
    std::vector<int64_t> lens64;
    for (auto &s : seqs) { lens.push_back(s.size()); lens64.push_back((int64_t)s.size()); }
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
        elba_place_stats st{};
        const elba::Placements pl = elba::place_reads(S, skip, &st);
        std::vector<int64_t> contig_lens;
        for (auto &s : contigs) contig_lens.push_back((int64_t)s.size());
        elba::write_placements_paf(argv[5], pl, names, lens64, contig_lens, &kinds);
        elba::write_gfa(argv[6], contigs, &kinds, elba::assembly_links(S), nullptr, &pl.credited_bases);
        std::ofstream rf(argv[7]);
        for (const elba_placement_t &p : pl.reads)
            rf << p.start << " " << p.contig << " " << p.anchor << " " << p.score << " " << (int)p.strand << " " << (int)p.kind << " " << (int)p.flags << "\n";
        for (size_t k = 0; k < contigs.size(); ++k) {
            rf << pl.seg_off[k + 1] - pl.seg_off[k] << " " << pl.credited_reads[k] << " " << pl.credited_bases[k] << "\n";
            for (int64_t j = pl.seg_off[k]; j < pl.seg_off[k + 1]; ++j) rf << pl.seg_start[(size_t)j] << " " << pl.seg_depth[(size_t)j] << "\n";
        }
        std::printf("{\"nreads\": %lld, \"chain\": %lld, \"anchored\": %lld, \"unanchored\": %lld, \"skipped\": %lld, \"empty\": %lld, \"candidates\": %lld, \"clipped\": %lld, "
                    "\"outside\": %lld, \"wrapped\": %lld, \"segments\": %lld, \"max_depth\": %lld, \"credited_bases\": %lld, \"contigs\": %zu}\n",
                    (long long)st.nreads, (long long)st.chain, (long long)st.anchored, (long long)st.unanchored, (long long)st.skipped, (long long)st.empty, (long long)st.candidates,
                    (long long)st.clipped, (long long)st.outside, (long long)st.wrapped, (long long)st.segments, (long long)st.max_depth, (long long)st.credited_bases, contigs.size());
    } catch (const elba::Error &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return e.status == ELBA_ERR_NO_DEVICE ? 3 : 1;
    }
    return 0;
}
