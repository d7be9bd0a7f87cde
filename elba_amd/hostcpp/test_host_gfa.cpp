// test_host_gfa.cpp — the assembly graph through the C++ mirror: reads + an edge list -> elba_set_overlaps -> elba_transitive_reduction ->
// GenerateContigs(flags, kinds) -> assembly_links -> write_gfa.  The edge list is text, one pair per line, ascending in (row, col):
//   row col direction directionT suffix suffixT
// LINKS receives one record per line (from to from_read to_read overlap from_rev to_rev flags).  Prints one JSON line of counts.
// Usage: test_host_gfa reads.fa edges.txt FLAGS out.gfa out.links [fuzz]
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include "elba_host.hpp"

int main(int argc, char **argv)
{
    if (argc < 6) { std::fprintf(stderr, "usage: %s reads.fa edges.txt FLAGS out.gfa out.links [fuzz]\n", argv[0]); return 2; }
    const int flags = std::atoi(argv[3]), fuzz = argc > 6 ? std::atoi(argv[6]) : 0;
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
    std::ifstream ein(argv[2]);
    long long r, c, d, dT, sfx, sfxT;
    while (ein >> r >> c >> d >> dT >> sfx >> sfxT) {
        elba_overlap_t o{};
        o.passed = 1; o.direction = (int8_t)d; o.directionT = (int8_t)dT; o.suffix = (int32_t)sfx; o.suffixT = (int32_t)sfxT;
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
        S.engine->check(elba_transitive_reduction(ctx, 0.0, fuzz, &S.stats));
        elba_contig_stats cst{};
        std::vector<uint8_t> kinds;
        std::vector<std::string> contigs = elba::GenerateContigs(S, mydna, &cst, flags, &kinds);
        elba_graph_stats st{};
        std::vector<elba_link_t> links = elba::assembly_links(S, &st);
        elba_contigs_t ec;
        S.engine->check(elba_export_contigs(ctx, &ec));
        std::vector<int64_t> chain_reads;
        for (int64_t i = 0; i < ec.n; ++i) chain_reads.push_back(ec.chain_off[i + 1] - ec.chain_off[i]);
        elba_free_contigs(&ec);
        elba::write_gfa(argv[4], contigs, &kinds, links, &chain_reads);
        std::ofstream lf(argv[5]);
        for (const elba_link_t &l : links)
            lf << l.from << " " << l.to << " " << l.from_read << " " << l.to_read << " " << l.overlap << " " << (int)l.from_rev << " " << (int)l.to_rev << " " << (int)l.flags << "\n";
        std::printf("{\"reads\": %zu, \"string_nnz\": %lld, \"records\": %zu, \"segments\": %lld, \"candidates\": %lld, \"links\": %lld, \"closures\": %lld, \"twisted\": %lld, "
                    "\"unplaced\": %lld, \"clamped\": %lld, \"asymmetric\": %lld}\n",
                    mydna.size(), (long long)S.stats.nnz, links.size(), (long long)st.segments, (long long)st.candidates, (long long)st.links, (long long)st.closures,
                    (long long)st.twisted, (long long)st.unplaced, (long long)st.clamped, (long long)st.asymmetric);
    } catch (const elba::Error &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return e.status == ELBA_ERR_NO_DEVICE ? 3 : 1;
    }
    return 0;
}
