// test_host_text.cpp — a FASTA or FASTQ file without a .fai -> reads on the context, written against elba_host.hpp (elba::set_reads_text).
// Prints one JSON line: reads, bases, lines, format, packed bytes, and checksums of the .fai records, the names and the packed bytes.
// Usage: test_host_text reads.{fa,fq}
#include "host_test.hpp"
namespace ht = elba::host_test;

int main(int argc, char **argv)
{
    return ht::run(argc, argv, 2, "reads.{fa,fq}", [&] {
        elba_cfg cfg{};
        cfg.k = 17; cfg.lower = 2; cfg.upper = 8;
        elba::detail::Engine engine(cfg);
        const elba::TextReads t = elba::set_reads_text(engine, argv[1]);
        unsigned long long rec_checksum = 0, name_checksum = 0, packed_checksum = 0;
        for (size_t i = 0; i < t.records.size(); ++i) {
            rec_checksum += (unsigned long long)(i + 1) * (t.records[i].len * 1000003ull + t.records[i].pos * 10007ull + t.records[i].bases);
            for (size_t j = 0; j < t.names[i].size(); ++j) name_checksum += (unsigned long long)(i + 1) * 131ull + (unsigned long long)(j + 1) * (unsigned char)t.names[i][j];
        }
        for (size_t b = 0; b < t.reads.getbufsize(); ++b) packed_checksum += (unsigned long long)(b + 1) * t.reads.data()[b];
        unsigned long long bases = 0;
        for (size_t i = 0; i < t.reads.size(); ++i) bases += t.reads.lengths()[i];
        ht::Json()("reads", t.reads.size())("bases", bases)("stat_bases", t.stats.bases)("lines", t.stats.lines)("format", t.stats.format)("packed_bytes", t.stats.packed_bytes)
            ("rec_checksum", rec_checksum)("name_checksum", name_checksum)("packed_checksum", packed_checksum).print();
        return 0;
    });
}
