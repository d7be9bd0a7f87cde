// host_test.hpp — what the stand-alone programs test_host_*.cpp share, and nothing a caller of elba_host.hpp needs: the FASTA reader, the
// front of the pipeline up to the string graph, the text forms of edge and pair lists, the comparison of a cleaned S with the S before it,
// the JSON line and the frame of main().  A program holds only what is its own: its arguments, its stage call, its host-side check, its
// output files and its JSON fields.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>
#include "elba_host.hpp"

namespace elba {
namespace host_test {

// The records of a FASTA file in file order: header lines without the '>', sequences with their lines joined, and the DnaBuffer of them.
// A record without bases is kept, as an empty read: read i here is read i of every other reader of the file.
struct Reads {
    std::vector<std::string> names, seqs;
    DnaBuffer dna;
    size_t size() const { return seqs.size(); }
};

inline Reads read_fasta(const std::string &path)
{
    Reads r;
    std::ifstream in(path);
    std::string line, cur;
    bool open = false;
    while (std::getline(in, line)) {
        if (!line.empty() && line[0] == '>') { if (open) r.seqs.push_back(cur); cur.clear(); open = true; r.names.push_back(line.substr(1)); }
        else cur += line;
    }
    if (open) r.seqs.push_back(cur);
    std::vector<size_t> lens;
    for (auto &s : r.seqs) lens.push_back(s.size());
    r.dna = DnaBuffer(DnaBuffer::computebufsize(lens));
    for (auto &s : r.seqs) r.dna.push_back(s.c_str(), s.size());
    return r;
}

// K LOWER UPPER, which follow the FASTA name on every pipeline program's command line
inline Params params_at(char **argv)
{
    Params prm;
    prm.kmer_size = std::atoi(argv[0]); prm.lower_kmer_freq = std::atoi(argv[1]); prm.upper_kmer_freq = std::atoi(argv[2]);
    return prm;
}

// src/main.cpp:191-312 on one rank: reads -> k-mers -> A -> B -> PairwiseAlignment -> TransitiveReduction, stopped where the caller says.
// What a program may still need stays reachable: kmermap (its engine is the one engine of the run; main.cpp:266 resets the map there, which
// frees nothing here, the counts being the engine's), A's sizes, B, R and S.  A k-mer map made another way (the FastaIndex ingest) may be
// handed in; the reads are then only the lengths PairwiseAlignment and TransitiveReduction read.
enum class Stop { B, R, S };

struct Front {
    std::unique_ptr<KmerCountMap> kmermap;
    int64_t nnzA = 0, ncol = 0;
    std::unique_ptr<SeedMatrix> B;
    std::unique_ptr<OverlapMatrix> R;
    std::unique_ptr<StringGraph> S;
};

inline Front run_to_string_graph(const Reads &reads, const Params &prm, double cutoff, Stop stop = Stop::S, std::unique_ptr<KmerCountMap> kmermap = nullptr)
{
    const DnaBuffer &mydna = reads.dna;
    auto commgrid = std::make_shared<Grid>();
    Front f;
    f.kmermap = kmermap ? std::move(kmermap) : get_kmer_count_map_keys(mydna, commgrid, prm);   // main.cpp:192
    get_kmer_count_map_values(mydna, *f.kmermap, commgrid);                                      // main.cpp:225
    auto A = create_kmer_matrix(mydna, *f.kmermap, commgrid);                                    // main.cpp:259
    auto AT = std::make_unique<KmerMatrix>(*A);                                                  // main.cpp:272-273
    AT->Transpose();
    f.B = create_seed_matrix(*A, *AT);                                                           // main.cpp:281
    f.nnzA = A->getnnz(); f.ncol = A->getncol();
    A.reset(); AT.reset();                                                                       // main.cpp:284-285
    if (stop == Stop::B) return f;
    // main.cpp:300 with the defaults of main.cpp:53-56
    f.R = PairwiseAlignment(mydna, *f.B, 1, -1, -1, 15);
    if (stop == Stop::R) return f;
    f.S = TransitiveReduction(mydna, *f.R, cutoff);                                              // main.cpp:305-312
    return f;
}

// Pairs as text, one per line, ascending in (row, col).  The edge list has six fields and describes pairs that passed:
//   row col direction directionT suffix suffixT
// the pair list has fifteen:
//   row col begQ endQ begT endT rc score passed containedQ containedT direction directionT suffix suffixT
struct Triples {
    std::vector<int64_t> rows, cols;
    std::vector<elba_overlap_t> vals;
};

inline Triples load_edges(const std::string &path)
{
    Triples t;
    std::ifstream in(path);
    long long r, c, d, dT, sfx, sfxT;
    while (in >> r >> c >> d >> dT >> sfx >> sfxT) {
        elba_overlap_t o{};
        o.passed = 1; o.direction = (int8_t)d; o.directionT = (int8_t)dT; o.suffix = (int32_t)sfx; o.suffixT = (int32_t)sfxT;
        t.rows.push_back(r); t.cols.push_back(c); t.vals.push_back(o);
    }
    return t;
}

inline Triples load_pairs(const std::string &path)
{
    Triples t;
    std::ifstream in(path);
    long long r, c, v[13];
    while (in >> r >> c) {
        for (long long &x : v) in >> x;
        elba_overlap_t o{};
        o.begQ = (int32_t)v[0]; o.endQ = (int32_t)v[1]; o.begT = (int32_t)v[2]; o.endT = (int32_t)v[3]; o.rc = (uint8_t)v[4]; o.score = (int32_t)v[5]; o.passed = (uint8_t)v[6];
        o.containedQ = (uint8_t)v[7]; o.containedT = (uint8_t)v[8]; o.direction = (int8_t)v[9]; o.directionT = (int8_t)v[10]; o.suffix = (int32_t)v[11]; o.suffixT = (int32_t)v[12];
        t.rows.push_back(r); t.cols.push_back(c); t.vals.push_back(o);
    }
    return t;
}

// The string graph of given pairs: a fresh engine (k = 17, lower = 2, upper = 8), the reads, elba_set_overlaps, elba_transitive_reduction with
// no bad-read cutoff.  S stays on the device; the host copy holds the stats only.
inline StringGraph loaded_graph(const Reads &reads, const std::vector<int64_t> &rows, const std::vector<int64_t> &cols, const std::vector<elba_overlap_t> &vals, int fuzz)
{
    const DnaBuffer &mydna = reads.dna;
    elba_cfg cfg{};
    cfg.k = 17; cfg.lower = 2; cfg.upper = 8;
    StringGraph S;
    S.numreads = (int64_t)mydna.size();
    S.engine = std::make_shared<detail::Engine>(cfg);
    elba_ctx *ctx = S.engine->ctx;
    S.engine->check(elba_set_reads(ctx, mydna.data(), mydna.offsets(), mydna.lengths(), (int64_t)mydna.size(), 0));
    S.engine->check(elba_set_overlaps(ctx, S.numreads, rows.data(), cols.data(), vals.data(), (int64_t)rows.size()));
    S.engine->check(elba_transitive_reduction(ctx, 0.0, fuzz, &S.stats));
    return S;
}

// What the tests compare with the binding's graph: sums over the entries of S, and over the reads a cleaning call removed.
inline unsigned long long s_checksum(const StringGraph &S)
{
    unsigned long long sum = 0;
    for (size_t a = 0; a < S.rows.size(); ++a)
        sum += (unsigned long long)(S.rows[a] + 1) * 1000003ull + (unsigned long long)S.cols[a] * 10007ull + (unsigned long long)(unsigned)S.vals[a].suffix;
    return sum;
}

inline unsigned long long read_checksum(const std::vector<int64_t> &removed)
{
    unsigned long long sum = 0;
    for (int64_t v : removed) sum += (unsigned long long)(v + 1) * 10007ull;
    return sum;
}

// Is S exactly the entries (rows0, cols0) that touch none of the reads `gone`, in their order?
inline bool kept_in_order(const std::vector<int64_t> &rows0, const std::vector<int64_t> &cols0, const std::vector<int64_t> &gone, const StringGraph &S)
{
    std::vector<uint8_t> is_gone((size_t)S.numreads, 0);
    for (int64_t v : gone) is_gone[(size_t)v] = 1;
    size_t at = 0;
    for (size_t a = 0; a < rows0.size(); ++a) {
        if (is_gone[(size_t)rows0[a]] || is_gone[(size_t)cols0[a]]) continue;
        if (at >= S.rows.size() || S.rows[at] != rows0[a] || S.cols[at] != cols0[a]) return false;
        ++at;
    }
    return at == S.rows.size();
}

// One line of JSON, the fields in the order given: j("reads", n)("pairs", m).print() writes {"reads": n, "pairs": m}.  Whole numbers only.
class Json {
public:
    template <class T>
    Json &operator()(const char *key, T value)
    {
        static_assert(std::is_integral<T>::value, "the JSON lines of the self-tests hold whole numbers");
        line_ += line_.empty() ? "{\"" : ", \"";
        line_ += key;
        line_ += "\": " + std::to_string(value);
        return *this;
    }
    void print() const { std::printf("%s}\n", line_.c_str()); }

private:
    std::string line_;
};

// The tail of the string-graph cleaning programs: GenerateContigs on the cleaned S, and its counts
inline void contig_counts(Json &j, StringGraph &S, const DnaBuffer &mydna)
{
    elba_contig_stats cs{};
    const std::vector<std::string> contigs = GenerateContigs(S, mydna, &cs);
    size_t bases = 0;
    for (auto &c : contigs) bases += c.size();
    j("contigs", contigs.size())("bases", bases)("branches", cs.branches);
}

// The frame of main(): too few arguments -> the usage line and status 2; an elba::Error from the body -> its text, and status 3 where there
// is no GPU, 1 otherwise; else the body's own status.
template <class Body>
int run(int argc, char **argv, int min_args, const char *usage, Body body)
{
    if (argc < min_args) { std::fprintf(stderr, "usage: %s %s\n", argv[0], usage); return 2; }
    try {
        return body();
    } catch (const Error &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return e.status == ELBA_ERR_NO_DEVICE ? 3 : 1;
    }
}

}  // namespace host_test
}  // namespace elba
