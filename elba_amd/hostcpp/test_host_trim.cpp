// test_host_trim.cpp — reads -> A -> B -> PairwiseAlignment -> GetReadPileup -> TrimReads -> AdoptTrimmedReads -> the k-mers of the pieces,
// written against elba_host.hpp; every base of every piece is held against the base of the source read the map names, and the unused
// bits of every piece's last byte against zero, on the host.
// Prints one JSON line: counts, checksums of the map and of the packed bytes, and whether the host comparison held.
// Usage: test_host_trim reads.fa K LOWER UPPER MODE MARGIN MIN_DEPTH MIN_RUN TRIM_LEN TRIM_MODE MIN_LEN
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include "elba_host.hpp"

int main(int argc, char **argv)
{
    if (argc < 12) { std::fprintf(stderr, "usage: %s reads.fa K LOWER UPPER MODE MARGIN MIN_DEPTH MIN_RUN TRIM_LEN TRIM_MODE MIN_LEN\n", argv[0]); return 2; }
    elba::Params prm;
    prm.kmer_size = std::atoi(argv[2]); prm.lower_kmer_freq = std::atoi(argv[3]); prm.upper_kmer_freq = std::atoi(argv[4]);
    elba_pileup_cfg cfg{};
    cfg.mode = std::atoi(argv[5]); cfg.margin = std::atoi(argv[6]); cfg.min_depth = std::atoi(argv[7]); cfg.min_run = std::atoi(argv[8]); cfg.trim_len = std::atoi(argv[9]);
    elba_trim_cfg tcfg{};
    tcfg.mode = std::atoi(argv[10]); tcfg.min_len = std::atoi(argv[11]);
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
        auto AT = std::make_unique<elba::KmerMatrix>(*A);
        AT->Transpose();
        auto B = elba::create_seed_matrix(*A, *AT);
        A.reset(); AT.reset();
        auto R = elba::PairwiseAlignment(mydna, *B, 1, -1, -1, 15);
        elba::GetReadPileup(mydna, *R, cfg);
        const elba_trim_stats st = elba::TrimReads(*R, tcfg);
        const elba::TrimMap map = elba::ExportTrimMap(*R);
        const elba::TrimmedReadsView view = elba::TrimmedReadsDevice(*R);
        const elba::DnaBuffer pieces = elba::AdoptTrimmedReads(*R);
        long long host_equal = (long long)map.size() == st.pieces && view.n == st.pieces && (long long)pieces.size() == st.pieces && view.packed_bytes == st.packed_bytes &&
                               (long long)pieces.getbufsize() == st.packed_bytes;
        unsigned long long map_checksum = 0, byte_checksum = 0, at = 0;
        for (size_t p = 0; p < map.size() && host_equal; ++p) {
            const size_t r = (size_t)map.src_read[p], b = (size_t)map.src_beg[p], L = (size_t)(map.src_end[p] - map.src_beg[p]);
            map_checksum += (unsigned long long)(r + 1) * 1000003ull + (unsigned long long)b * 10007ull + (unsigned long long)map.src_end[p];
            if (pieces.lengths()[p] != L || pieces.offsets()[p] != at) host_equal = 0;
            for (size_t i = 0; i < L && host_equal; ++i) if (pieces.base(p, i) != mydna.base(r, b + i)) host_equal = 0;
            for (size_t i = L; i < 4 * elba::DnaBuffer::bytesneeded(L) && host_equal; ++i) if (pieces.base(p, i) != 0) host_equal = 0;
            at += elba::DnaBuffer::bytesneeded(L);
        }
        for (size_t i = 0; i < pieces.getbufsize(); ++i) byte_checksum += (unsigned long long)pieces.data()[i] * (i % 1000003ull + 1);
        // the engine holds the pieces now: the k-mer stage runs on them
        elba_kmer_stats ks{};
        kmermap->engine->check(elba_count_kmers(kmermap->engine->ctx, &ks));
        std::printf("{\"reads\": %zu, \"pieces\": %lld, \"reads_split\": %lld, \"reads_dropped\": %lld, \"bases_out\": %lld, \"packed_bytes\": %lld, \"map_checksum\": %llu, "
                    "\"byte_checksum\": %llu, \"host_equal\": %lld, \"kmer_reads\": %lld, \"kmer_instances\": %lld}\n",
                    mydna.size(), (long long)st.pieces, (long long)st.reads_split, (long long)st.reads_dropped, (long long)st.bases_out, (long long)st.packed_bytes, map_checksum,
                    byte_checksum, host_equal, (long long)ks.nreads, (long long)ks.instances);
    } catch (const elba::Error &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return e.status == ELBA_ERR_NO_DEVICE ? 3 : 1;
    }
    return 0;
}
