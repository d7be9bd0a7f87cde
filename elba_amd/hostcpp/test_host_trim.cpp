// test_host_trim.cpp — reads -> A -> B -> PairwiseAlignment -> GetReadPileup -> TrimReads -> AdoptTrimmedReads -> the k-mers of the pieces,
// written against elba_host.hpp; every base of every piece is held against the base of the source read the map names, and the unused
// bits of every piece's last byte against zero, on the host.
// Prints one JSON line: counts, checksums of the map and of the packed bytes, and whether the host comparison held.
// Usage: test_host_trim reads.fa K LOWER UPPER MODE MARGIN MIN_DEPTH MIN_RUN TRIM_LEN TRIM_MODE MIN_LEN
#include "host_test.hpp"
namespace ht = elba::host_test;

int main(int argc, char **argv)
{
    return ht::run(argc, argv, 12, "reads.fa K LOWER UPPER MODE MARGIN MIN_DEPTH MIN_RUN TRIM_LEN TRIM_MODE MIN_LEN", [&] {
        elba_pileup_cfg cfg{};
        cfg.mode = std::atoi(argv[5]); cfg.margin = std::atoi(argv[6]); cfg.min_depth = std::atoi(argv[7]); cfg.min_run = std::atoi(argv[8]); cfg.trim_len = std::atoi(argv[9]);
        elba_trim_cfg tcfg{};
        tcfg.mode = std::atoi(argv[10]); tcfg.min_len = std::atoi(argv[11]);
        const ht::Reads reads = ht::read_fasta(argv[1]);
        const elba::DnaBuffer &mydna = reads.dna;
        const ht::Front f = ht::run_to_string_graph(reads, ht::params_at(argv + 2), 0.65, ht::Stop::R);
        elba::OverlapMatrix &R = *f.R;
        elba::GetReadPileup(mydna, R, cfg);
        const elba_trim_stats st = elba::TrimReads(R, tcfg);
        const elba::TrimMap map = elba::ExportTrimMap(R);
        const elba::TrimmedReadsView view = elba::TrimmedReadsDevice(R);
        const elba::DnaBuffer pieces = elba::AdoptTrimmedReads(R);
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
        f.kmermap->engine->check(elba_count_kmers(f.kmermap->engine->ctx, &ks));
        ht::Json()("reads", reads.size())("pieces", st.pieces)("reads_split", st.reads_split)("reads_dropped", st.reads_dropped)("bases_out", st.bases_out)
            ("packed_bytes", st.packed_bytes)("map_checksum", map_checksum)("byte_checksum", byte_checksum)("host_equal", host_equal)("kmer_reads", ks.nreads)
            ("kmer_instances", ks.instances).print();
        return 0;
    });
}
