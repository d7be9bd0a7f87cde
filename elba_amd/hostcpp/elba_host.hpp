// elba_host.hpp — C++17 host-side mirror of the reference's operator surface for the overlap hot path, over the C ABI of
// include/elba_amd.h.  Same function names, argument meaning and ownership conventions as the reference so that
// src/main.cpp:191-300 reads the same with `elba::` types in place of the CombBLAS ones:
//
//   reference                                                        this header
//   ---------------------------------------------------------------  --------------------------------------------------
//   DnaBuffer            include/DnaBuffer.hpp:13-38                  elba::DnaBuffer   (same 2-bit layout, src/DnaSeq.cpp:7-29)
//   KmerCountMap         include/KmerOps.hpp:22                       elba::KmerCountMap (opaque: the counts live in HBM)
//   get_kmer_count_map_keys / _values   include/KmerOps.hpp:27-30     same names
//   create_kmer_matrix   include/KmerOps.hpp:24-25                    same name -> elba::KmerMatrix (CSR and CSC both resident)
//   AT = *A; AT->Transpose()            src/main.cpp:272-273          KmerMatrix copy + Transpose(): no work, both orientations exist
//   SharedSeeds          include/SharedSeeds.hpp:8-96                 elba::SharedSeeds (same members and accessors)
//   create_seed_matrix   include/SharedSeeds.hpp:98-99                same name -> elba::SeedMatrix
//   FastaIndex           include/FastaIndex.hpp, src/FastaIndex.cpp          same name: .fai records, base-balanced partition, chunk bounds;
//                                                                             the reads are 2-bit encoded on the GPU (elba_set_reads_fasta)
//   (none: the reference reads only indexed FASTA)                            elba::set_reads_text(engine, path): FASTA or FASTQ text without a .fai,
//                                                                             indexed and encoded on the GPU (elba_set_reads_text)
//   PairwiseAlignment    include/PairwiseAlignment.hpp, src/PairwiseAlignment.cpp:5-106     same name -> elba::OverlapMatrix (triples of elba::Overlap)
//   Bmat.seqptr()->getnnz() / GetDCSC()  src/PairwiseAlignment.cpp:16-19   SeedMatrix::seqptr()->getnnz() / GetDCSC()
//   find_bad_reads / find_contained_reads / TransitiveReduction   src/main.cpp:305-312, src/TransitiveReduction.cpp:3-90
//                                                                             elba::TransitiveReduction(R, cutoff): the prunes and the reduction in one
//                                                                             call on the GPU -> elba::StringGraph (S + the two read lists)
//   GenerateContigs / parallel_write_contigs   src/ContigGeneration.cpp:376-457, src/main.cpp:487-512   same names (one rank): the contigs are
//                                                                             built on the GPU from the S left there
//   (none: the reference drops every branch read)                             elba::ClipTips(S, reads, max_tip_reads, rounds): dead-end tips leave S
//   (none)                                                                    elba::PopBubbles(S, reads, max_arm_reads, rounds): all but one arm of a bubble leave S
//   (none)                                                                    elba::CutWeakOverlaps(S, reads, min_ratio_q16): weak overlaps at branching read ends leave S
//   asmtools/bridge_removal.py (a script run on the written-out graph)        elba::CutBridges(S, reads, max_bridge_reads, min_flank_reads): short chains between two long paths leave S
//   asmtools/star_resolution.py (a script run on the written-out graphs)      elba::ResolveStars(S, reads, rounds): the stray arm of a three-armed star leaves S
//   (not in the reference: reads-to-contigs PAF, depth per contig)             elba::place_reads(S) + elba::write_placements_paf(...), write_gfa(..., depth)
//   asmtools/create_gml.py, assemble_gml.py (scripts over the PAF files)      elba::assembly_links(S) + elba::write_gfa(...): the contigs as segments and the
//                                                                             edges of S at branch reads as links, found on the GPU, written as GFA 1
//
// Errors: the reference asserts/aborts; here every failing C-ABI status throws elba::Error (status + text).
// There is no CPU path: constructing an engine without a GPU throws ELBA_ERR_NO_DEVICE.
#pragma once
#include <cstdint>
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <ostream>
#include <memory>
#include <sstream>
#include <stdexcept>
#include <string>
#include <tuple>
#include <vector>
#include "../../include/elba_amd.h"

namespace elba {

using PosInRead = uint32_t;   // include/KmerOps.hpp:14
using ReadId = int64_t;       // include/KmerOps.hpp:15

struct Error : std::runtime_error {
    int status;
    Error(int s, const std::string &t) : std::runtime_error("elba status " + std::to_string(s) + ": " + t), status(s) {}
};

// The process grid argument of the reference (std::shared_ptr<CommGrid>): one rank per GPU, 1D here.
struct Grid {
    int rank = 0, size = 1, device = 0;
    int GetRank() const { return rank; }
    int GetSize() const { return size; }
};

// 2-bit read buffer, 4 bases per byte, first base in bits 7-6, reads byte-aligned (src/DnaSeq.cpp:7-29, src/DnaBuffer.cpp:22-29).
class DnaBuffer {
public:
    static size_t bytesneeded(size_t n) { return (n + 3) / 4; }                       // include/DnaSeq.hpp:131
    static size_t computebufsize(const std::vector<size_t> &lens)
    {
        size_t s = 0;
        for (size_t l : lens) s += bytesneeded(l);
        return s;
    }
    explicit DnaBuffer(size_t bufsize = 0) { buf_.reserve(bufsize + 16); }
    void push_back(char const *s, size_t len)
    {
        const size_t nb = bytesneeded(len), at = buf_.size();
        buf_.resize(at + nb, 0);
        for (size_t i = 0; i < len; ++i) buf_[at + i / 4] |= (uint8_t)(code(s[i]) << (6 - 2 * (i % 4)));
        off_.push_back(at);
        len_.push_back((uint32_t)len);
    }
    size_t size() const { return len_.size(); }
    size_t getbufsize() const { return buf_.size(); }
    const uint8_t *data() const { return buf_.data(); }
    const uint64_t *offsets() const { return off_.data(); }
    const uint32_t *lengths() const { return len_.data(); }
    int base(size_t read, size_t i) const { return (buf_[off_[read] + i / 4] >> (6 - 2 * (i % 4))) & 3; }   // DnaSeq::operator[]
    // a buffer that exists in this layout already (elba_export_reads): packed bytes, byte offsets, lengths
    static DnaBuffer from_packed(std::vector<uint8_t> buf, std::vector<uint64_t> off, std::vector<uint32_t> len)
    {
        DnaBuffer d;
        d.buf_ = std::move(buf); d.off_ = std::move(off); d.len_ = std::move(len);
        return d;
    }

private:
    static uint8_t code(char c)                                                        // include/DnaSeq.hpp:136-154
    {
        switch (c) {
        case 'A': case 'a': case 'N': case 'n': return 0;
        case 'C': case 'c': return 1;
        case 'G': case 'g': return 2;
        case 'T': case 't': return 3;
        default: return 4;
        }
    }
    std::vector<uint8_t> buf_;
    std::vector<uint64_t> off_;
    std::vector<uint32_t> len_;
};

// include/FastaIndex.hpp — the host side of the ingest: the .fai next to the FASTA (`name len pos bases [width]`, src/FastaIndex.cpp:15-23), the
// greedy base-balanced contiguous partition (:47-94: a rank takes reads while the next one keeps it under total / nprocs, the last rank
// the rest) and the bytes of the file a rank needs (:222-224).  What getmydna does after reading that chunk — stripping line ends and
// DnaSeq::compress — runs on the GPU instead: get_kmer_count_map_keys(index, ...) below hands the raw chunk to elba_set_reads_fasta.
class FastaIndex {
public:
    typedef elba_fasta_record_t Record;                       // {len, pos, bases}: FastaIndex::Record, include/FastaIndex.hpp:10
    FastaIndex(const std::string &fasta_fname, std::shared_ptr<Grid> commgrid) : commgrid(commgrid), fasta_fname(fasta_fname)
    {
        std::ifstream in(get_faidx_fname());
        if (!in) throw Error(ELBA_ERR_INVALID_ARG, "cannot open " + get_faidx_fname());
        std::string line, name;
        while (std::getline(in, line)) {
            std::istringstream ls(line);
            Record r{};
            if (!(ls >> name >> r.len >> r.pos >> r.bases)) continue;      // get_faidx_record, src/FastaIndex.cpp:15-23
            rootrecords.push_back(r); rootnames.push_back(name);
        }
        const int nprocs = commgrid->GetSize();
        size_t totbases = 0;
        for (auto &r : rootrecords) totbases += r.len;
        const double avg = (double)totbases / nprocs;
        readdispls.assign((size_t)nprocs + 1, 0);
        size_t at = 0;
        for (int i = 0; i < nprocs - 1; ++i) {                               // getpartition, src/FastaIndex.cpp:47-94
            size_t sofar = 0;
            while (at < rootrecords.size() && sofar + rootrecords[at].len < avg) sofar += rootrecords[at++].len;
            readdispls[(size_t)i + 1] = at;
        }
        readdispls[(size_t)nprocs] = rootrecords.size();
        const size_t lo = readdispls[(size_t)commgrid->GetRank()], hi = readdispls[(size_t)commgrid->GetRank() + 1];
        myrecords.assign(rootrecords.begin() + (std::ptrdiff_t)lo, rootrecords.begin() + (std::ptrdiff_t)hi);
    }
    std::string get_fasta_fname() const { return fasta_fname; }
    std::string get_faidx_fname() const { return fasta_fname + ".fai"; }
    size_t gettotrecords() const { return rootrecords.size(); }
    size_t getmyreadcount() const { return myrecords.size(); }
    size_t getmyreaddispl() const { return readdispls[(size_t)commgrid->GetRank()]; }
    const std::vector<Record> &getmyrecords() const { return myrecords; }
    const std::vector<size_t> &getreaddispls() const { return readdispls; }
    const std::vector<std::string> &getnames() const { return rootnames; }
    std::shared_ptr<Grid> getcommgrid() const { return commgrid; }
    // the raw bytes of the file that hold this rank's records, and the file offset of the first one (src/FastaIndex.cpp:222-241)
    std::vector<char> readmychunk(uint64_t &startpos) const
    {
        std::vector<char> buf;
        startpos = 0;
        if (myrecords.empty()) return buf;
        std::ifstream in(fasta_fname, std::ios::binary | std::ios::ate);
        if (!in) throw Error(ELBA_ERR_INVALID_ARG, "cannot open " + fasta_fname);
        const uint64_t filesize = (uint64_t)in.tellg();
        startpos = myrecords.front().pos;
        uint64_t endpos = myrecords.back().pos + myrecords.back().len + myrecords.back().len / myrecords.back().bases;
        if (endpos > filesize) endpos = filesize;
        buf.resize((size_t)(endpos - startpos));
        in.seekg((std::streamoff)startpos);
        in.read(buf.data(), (std::streamsize)buf.size());
        return buf;
    }

private:
    std::shared_ptr<Grid> commgrid;
    std::vector<Record> myrecords, rootrecords;
    std::vector<size_t> readdispls;
    std::vector<std::string> rootnames;
    std::string fasta_fname;
};

// include/SharedSeeds.hpp:8-96 — same members, constructors and accessors (the Semiring runs on the GPU).
struct SharedSeeds {
    SharedSeeds() : numshared(0) {}
    SharedSeeds(PosInRead begQ, PosInRead begT) : numshared(1) { std::get<0>(seeds[0]) = begQ; std::get<1>(seeds[0]) = begT; }
    SharedSeeds(const std::tuple<PosInRead, PosInRead> &s1, const std::tuple<PosInRead, PosInRead> &s2, int n) : numshared(n) { seeds[0] = s1; seeds[1] = s2; }
    explicit SharedSeeds(const elba_seed_t &v) : numshared(v.numshared)               // field-wise: never memcpy
    {
        std::get<0>(seeds[0]) = v.q0; std::get<1>(seeds[0]) = v.t0;
        std::get<0>(seeds[1]) = v.q1; std::get<1>(seeds[1]) = v.t1;
    }
    int getnumstored() const { return numshared < 2 ? numshared : 2; }
    int getnumshared() const { return numshared; }
    const std::tuple<PosInRead, PosInRead> *getseeds() const { return &seeds[0]; }
    std::tuple<PosInRead, PosInRead> seeds[2];
    int numshared;
};

namespace detail {
struct Engine {
    elba_ctx *ctx = nullptr;
    explicit Engine(const elba_cfg &cfg)
    {
        int rc = elba_ctx_create(&ctx, &cfg);
        if (rc != ELBA_OK) throw Error(rc, elba_strerror(rc));
    }
    ~Engine() { elba_ctx_destroy(ctx); }
    Engine(const Engine &) = delete;
    Engine &operator=(const Engine &) = delete;
    void check(int rc) const { if (rc != ELBA_OK) throw Error(rc, std::string(elba_strerror(rc)) + ": " + elba_last_error(ctx)); }
};
}  // namespace detail

// Compile-time constants of the reference (Makefile:1-6, include/compiletime.h) are run-time parameters here.
struct Params {
    int kmer_size = 31, lower_kmer_freq = 15, upper_kmer_freq = 35;
};

class KmerCountMap {
public:
    std::shared_ptr<detail::Engine> engine;
    elba_kmer_stats stats{};
    size_t size() const { return (size_t)stats.reliable; }       // reliable 'column' k-mers (src/KmerOps.cpp:343-346)
};

// What the reference's CT<SharedSeeds>::PSpDCCols exposes to PairwiseAlignment (src/PairwiseAlignment.cpp:16-32).
struct Dcsc {
    int64_t nzc = 0;
    std::vector<int64_t> jc, cp, ir;
    std::vector<SharedSeeds> numx;
};

class SeqSeedMatrix {
public:
    int64_t getnnz() const { return (int64_t)dcsc_.numx.size(); }
    const Dcsc *GetDCSC() const { return getnnz() ? &dcsc_ : nullptr; }
    Dcsc dcsc_;
};

class SeedMatrix {
public:
    std::shared_ptr<detail::Engine> engine;
    elba_overlap_stats stats{};
    int64_t nrows = 0;
    int64_t getnnz() const { return stats.nnz; }
    int64_t getnrow() const { return nrows; }
    int64_t getncol() const { return nrows; }
    // local block of this rank's grid cell; one rank: the whole matrix
    const SeqSeedMatrix *seqptr()
    {
        if (!seq_) {
            elba_dcsc_t d;
            engine->check(elba_export_dcsc(engine->ctx, 0, nrows, 0, nrows, &d));
            seq_ = std::make_unique<SeqSeedMatrix>();
            Dcsc &o = seq_->dcsc_;
            o.nzc = d.nzc;
            o.jc.assign(d.jc, d.jc + d.nzc);
            o.cp.assign(d.cp, d.cp + d.nzc + 1);
            o.ir.assign(d.ir, d.ir + d.nnz);
            o.numx.reserve((size_t)d.nnz);
            for (int64_t i = 0; i < d.nnz; ++i) o.numx.emplace_back(d.numx[i]);
            elba_free_dcsc(&d);
        }
        return seq_.get();
    }

private:
    std::unique_ptr<SeqSeedMatrix> seq_;
};

class KmerMatrix {
public:
    std::shared_ptr<detail::Engine> engine;
    elba_matrix_stats stats{};
    int64_t getnrow() const { return stats.nrows; }
    int64_t getncol() const { return stats.ncols; }
    int64_t getnnz() const { return stats.nnz; }
    void Transpose() {}        // CSR and CSC of A are both resident on the device: AT is a view, not a copy (src/main.cpp:272-273)
};

inline std::unique_ptr<KmerCountMap> get_kmer_count_map_keys(const DnaBuffer &myreads, std::shared_ptr<Grid> grid, const Params &prm = Params())
{
    if (grid->GetSize() != 1) throw Error(ELBA_ERR_UNSUPPORTED, "the C++ mirror drives one GPU; multi-GPU runs go through the elba_dist_* entry points");
    elba_cfg cfg{};
    cfg.k = prm.kmer_size; cfg.lower = prm.lower_kmer_freq; cfg.upper = prm.upper_kmer_freq; cfg.device = grid->device;
    auto map = std::make_unique<KmerCountMap>();
    map->engine = std::make_shared<detail::Engine>(cfg);
    map->engine->check(elba_set_reads(map->engine->ctx, myreads.data(), myreads.offsets(), myreads.lengths(), (int64_t)myreads.size(), 0));
    // both passes of the reference (keys: src/KmerOps.cpp:18-204, values: :206-350) are one exact count on the GPU
    map->engine->check(elba_count_kmers(map->engine->ctx, &map->stats));
    return map;
}

// The same entry point for a caller that has not parsed its reads yet: the rank's chunk of the FASTA goes to the GPU as it is in the file.
// index.getmydna()'s result can still be had from the context (elba_export_reads) — e.g. for the lengths PairwiseAlignment needs: `reads` is
// filled with them here (the mirror's DnaBuffer keeps lengths and offsets; the packed bytes are fetched only on demand).
inline std::unique_ptr<KmerCountMap> get_kmer_count_map_keys(const FastaIndex &index, std::shared_ptr<Grid> grid, const Params &prm, elba_ingest_stats *ingest = nullptr)
{
    if (grid->GetSize() != 1) throw Error(ELBA_ERR_UNSUPPORTED, "the C++ mirror drives one GPU; multi-GPU runs go through the elba_dist_* entry points");
    elba_cfg cfg{};
    cfg.k = prm.kmer_size; cfg.lower = prm.lower_kmer_freq; cfg.upper = prm.upper_kmer_freq; cfg.device = grid->device;
    auto map = std::make_unique<KmerCountMap>();
    map->engine = std::make_shared<detail::Engine>(cfg);
    uint64_t startpos = 0;
    const std::vector<char> chunk = index.readmychunk(startpos);
    elba_ingest_stats is{};
    map->engine->check(elba_set_reads_fasta(map->engine->ctx, chunk.data(), (int64_t)chunk.size(), startpos, index.getmyrecords().data(),
                                            (int64_t)index.getmyreadcount(), (int64_t)index.getmyreaddispl(), &is));
    if (ingest) *ingest = is;
    map->engine->check(elba_count_kmers(map->engine->ctx, &map->stats));
    return map;
}

// Reads from a FASTA or FASTQ file that has no .fai: the whole file goes to the GPU as text, the index is built there (elba_set_reads_text)
// and comes back with the reads — the names (sliced here from the file's bytes), the .fai records, and the reads in DnaBuffer layout as
// index.getmydna() would have left them.  Mirrors Engine.set_reads_file / export_read_index of the Python binding; a .gz is not inflated here.
struct TextReads {
    std::vector<std::string> names;
    std::vector<elba_fasta_record_t> records;
    DnaBuffer reads;
    elba_text_stats stats{};
};
inline TextReads set_reads_text(detail::Engine &engine, const std::string &path, int format = ELBA_TEXT_AUTO, int64_t first_global_id = 0)
{
    std::ifstream in(path, std::ios::binary);
    if (!in) throw Error(ELBA_ERR_INVALID_ARG, "cannot open " + path);
    const std::string text((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    elba_text_cfg cfg{};
    cfg.format = format; cfg.first_global_id = first_global_id;
    TextReads out;
    engine.check(elba_set_reads_text(engine.ctx, text.data(), (int64_t)text.size(), 0, &cfg, &out.stats));
    const size_t m = (size_t)out.stats.nreads;
    std::vector<uint64_t> name_pos(m), off(m);
    std::vector<uint32_t> name_len(m), len(m);
    std::vector<uint8_t> buf((size_t)out.stats.packed_bytes);
    out.records.resize(m);
    engine.check(elba_export_read_index(engine.ctx, out.records.data(), name_pos.data(), name_len.data(), (int64_t)m));
    engine.check(elba_export_reads(engine.ctx, buf.data(), out.stats.packed_bytes, off.data(), len.data(), (int64_t)m));
    out.names.reserve(m);
    for (size_t i = 0; i < m; ++i) out.names.emplace_back(text, (size_t)name_pos[i], (size_t)name_len[i]);
    out.reads = DnaBuffer::from_packed(std::move(buf), std::move(off), std::move(len));
    return out;
}

inline void get_kmer_count_map_values(const DnaBuffer &, KmerCountMap &kmermap, std::shared_ptr<Grid>)
{
    if (!kmermap.engine) throw Error(ELBA_ERR_STATE, "get_kmer_count_map_values: empty k-mer map");
}

inline std::unique_ptr<KmerMatrix> create_kmer_matrix(const DnaBuffer &, const KmerCountMap &kmermap, std::shared_ptr<Grid>)
{
    auto A = std::make_unique<KmerMatrix>();
    A->engine = kmermap.engine;
    A->engine->check(elba_create_kmer_matrix(A->engine->ctx, &A->stats));
    return A;
}

inline std::unique_ptr<SeedMatrix> create_seed_matrix(KmerMatrix &A, KmerMatrix &AT)
{
    if (A.engine != AT.engine) throw Error(ELBA_ERR_INVALID_ARG, "create_seed_matrix: A and AT must come from the same create_kmer_matrix");
    auto B = std::make_unique<SeedMatrix>();
    B->engine = A.engine;
    B->nrows = A.stats.nrows;
    B->engine->check(elba_create_seed_matrix(B->engine->ctx, &B->stats));   // Mult_AnXBn_DoubleBuff + Prune(numshared <= 1), src/SharedSeeds.cpp:7-8
    return B;
}

// The fields of the reference's Overlap that extend_overlap fills (include/Overlap.hpp:22-28; src/Overlap.cpp:24-73), same names.
struct Overlap {
    std::tuple<PosInRead, PosInRead> beg, end, len, seed;
    int score = 0, suffix = 0, suffixT = 0;
    int8_t direction = -1, directionT = -1;
    bool rc = false, passed = false, containedQ = false, containedT = false;
};

// What PairwiseAlignment hands to SpParMat<Overlap>(numreads, numreads, drows, dcols, dvals, false): the local triples (src/PairwiseAlignment.cpp:97-103)
class OverlapMatrix {
public:
    int64_t numreads = 0;
    std::vector<int64_t> rows, cols;
    std::vector<Overlap> vals;
    elba_align_stats stats{};
    std::shared_ptr<detail::Engine> engine;  // the alignments stay on the device for the string-graph stage
    int64_t getnnz() const { return (int64_t)vals.size(); }
};

namespace detail {
// One exported pair as the reference's Overlap.  (Overlap::seed, a copy of seeds[0] of B(i,j), is not carried back: the caller still owns B)
inline Overlap to_overlap(const elba_overlap_t &v, PosInRead lenQ, PosInRead lenT)
{
    Overlap w;
    w.beg = std::make_tuple((PosInRead)v.begQ, (PosInRead)v.begT); w.end = std::make_tuple((PosInRead)v.endQ, (PosInRead)v.endT);
    w.len = std::make_tuple(lenQ, lenT);
    w.score = v.score; w.suffix = v.suffix; w.suffixT = v.suffixT; w.direction = v.direction; w.directionT = v.directionT;
    w.rc = v.rc; w.passed = v.passed; w.containedQ = v.containedQ; w.containedT = v.containedT;
    return w;
}

// The triples of an export (elba_export_overlaps, elba_export_string_graph) into rows, cols and vals; the export is freed, also when a copy throws.
inline void take_triples(elba_overlaps_t &o, const DnaBuffer &myreads, std::vector<int64_t> &rows, std::vector<int64_t> &cols, std::vector<Overlap> &vals)
{
    try {
        rows.assign(o.rows, o.rows + o.n); cols.assign(o.cols, o.cols + o.n);
        vals.clear();
        vals.reserve((size_t)o.n);
        for (int64_t a = 0; a < o.n; ++a) vals.push_back(to_overlap(o.vals[a], (PosInRead)myreads.lengths()[o.rows[a]], (PosInRead)myreads.lengths()[o.cols[a]]));
    } catch (...) {
        elba_free_overlaps(&o);
        throw;
    }
    elba_free_overlaps(&o);
}
}  // namespace detail

// PairwiseAlignment(dfd, Bmat, mat, mis, gap, dropoff) — src/PairwiseAlignment.cpp:5-106 on one rank: every stored B(i,j), i < j, is
// aligned from seeds[0] on the GPU (the reads are the ones the k-mer stage was given; DistributedFastaData's row/column buffers are
// the same buffer on one rank).
inline std::unique_ptr<OverlapMatrix> PairwiseAlignment(const DnaBuffer &myreads, SeedMatrix &Bmat, int mat, int mis, int gap, int dropoff)
{
    auto R = std::make_unique<OverlapMatrix>();
    R->numreads = Bmat.getnrow();
    R->engine = Bmat.engine;
    Bmat.engine->check(elba_align_seeds(Bmat.engine->ctx, mat, mis, gap, dropoff, &R->stats));
    elba_overlaps_t o;
    Bmat.engine->check(elba_export_overlaps(Bmat.engine->ctx, &o));
    detail::take_triples(o, myreads, R->rows, R->cols, R->vals);
    return R;
}

// The string graph S of src/main.cpp:312 with what main() derives on the way: the reads find_bad_reads (:305) and find_contained_reads
// (:310) return.  Entries in the order parallel_write_paf walks S (:527-541): columns ascending, rows ascending within a column.
class StringGraph {
public:
    int64_t numreads = 0;
    std::vector<int64_t> rows, cols;
    std::vector<Overlap> vals;
    std::vector<int64_t> bad_reads, contained_reads;
    elba_string_stats stats{};
    std::shared_ptr<detail::Engine> engine;  // S stays on the device for the contig stage
    int64_t getnnz() const { return (int64_t)vals.size(); }
};

// src/main.cpp:305-312 — bad_reads = find_bad_reads(*R, cutoff); R->Prune(!passed); R->PruneFull(bad_reads, bad_reads);
// contained = find_contained_reads(*R); R->PruneFull(contained, contained); S = TransitiveReduction(*R) — as one call on the
// alignments PairwiseAlignment left on the device.  R itself is not modified (the reference prunes it in place and then drops it).
inline std::unique_ptr<StringGraph> TransitiveReduction(const DnaBuffer &myreads, OverlapMatrix &R, double bad_read_cutoff, int fuzz = 1000)
{
    auto S = std::make_unique<StringGraph>();
    S->numreads = R.numreads;
    S->engine = R.engine;
    R.engine->check(elba_transitive_reduction(R.engine->ctx, bad_read_cutoff, fuzz, &S->stats));
    elba_overlaps_t o;
    R.engine->check(elba_export_string_graph(R.engine->ctx, &o));
    detail::take_triples(o, myreads, S->rows, S->cols, S->vals);
    std::vector<uint8_t> flags((size_t)R.numreads);
    R.engine->check(elba_export_read_flags(R.engine->ctx, flags.data(), R.numreads));
    for (int64_t v = 0; v < R.numreads; ++v) {
        if (flags[(size_t)v] & 1) S->bad_reads.push_back(v);
        if (flags[(size_t)v] & 2) S->contained_reads.push_back(v);
    }
    return S;
}

// The host copy of S after a call that changed it on the device (ClipTips, PopBubbles, CutWeakOverlaps, CutBridges, ResolveStars): the entries of elba_export_string_graph; removed_reads,
// if given, receives the reads that carry `flag` in elba_export_read_flags, ascending.
inline void reload_string_graph(StringGraph &S, const DnaBuffer &myreads, uint8_t flag, std::vector<int64_t> *removed_reads)
{
    elba_overlaps_t o;
    S.engine->check(elba_export_string_graph(S.engine->ctx, &o));
    detail::take_triples(o, myreads, S.rows, S.cols, S.vals);
    if (removed_reads) {
        std::vector<uint8_t> flags((size_t)S.numreads);
        S.engine->check(elba_export_read_flags(S.engine->ctx, flags.data(), S.numreads));
        removed_reads->clear();
        for (int64_t v = 0; v < S.numreads; ++v) if (flags[(size_t)v] & flag) removed_reads->push_back(v);
    }
}

// What the five cleaning calls below share: S must be on a device; fn(ctx, &cfg, &stats) changes it there; the host copy is reloaded, with the
// reads that carry `flag` into `removed`.
namespace detail {
template <class Stats, class Cfg, class Fn>
inline Stats clean_call(StringGraph &S, const DnaBuffer &myreads, const char *who, uint8_t flag, std::vector<int64_t> *removed, Fn fn, const Cfg &cfg)
{
    if (!S.engine) throw Error(ELBA_ERR_STATE, std::string(who) + ": the string graph is not on a device");
    Stats st{};
    S.engine->check(fn(S.engine->ctx, &cfg, &st));
    reload_string_graph(S, myreads, flag, removed);
    return st;
}
}  // namespace detail

// ClipTips(S, myreads, max_tip_reads, rounds) — not in the reference: elba_clip_tips on the S that TransitiveReduction left on the device, between
// that call and GenerateContigs.  Dead-end chains of at most max_tip_reads reads that hang off a read of degree >= 3 leave S (a star of nothing
// but such chains is spared), in up to `rounds` rounds; the host copy of S is replaced by the clipped graph, and clipped_reads, if given,
// receives the reads removed so far (flag bit 2 of elba_export_read_flags), ascending.
inline elba_tip_stats ClipTips(StringGraph &S, const DnaBuffer &myreads, int max_tip_reads, int rounds = 1, std::vector<int64_t> *clipped_reads = nullptr)
{
    elba_tip_cfg cfg{};
    cfg.max_tip_reads = max_tip_reads; cfg.rounds = rounds;
    return detail::clean_call<elba_tip_stats>(S, myreads, "ClipTips", 4, clipped_reads, elba_clip_tips, cfg);
}

// PopBubbles(S, myreads, max_arm_reads, rounds) — not in the reference: elba_pop_bubbles on the S that TransitiveReduction (or ClipTips) left on the
// device, before GenerateContigs.  Where two or more chains of at most max_arm_reads reads of degree 2 join the same two reads of degree >= 3,
// the one with the most reads stays (on a tie the one whose first read is smallest) and the others leave S, in up to `rounds` rounds; the host
// copy of S is replaced by the popped graph, and popped_reads, if given, receives the reads removed so far (flag bit 3 of
// elba_export_read_flags), ascending.
inline elba_bubble_stats PopBubbles(StringGraph &S, const DnaBuffer &myreads, int max_arm_reads, int rounds = 1, std::vector<int64_t> *popped_reads = nullptr)
{
    elba_bubble_cfg cfg{};
    cfg.max_arm_reads = max_arm_reads; cfg.rounds = rounds;
    return detail::clean_call<elba_bubble_stats>(S, myreads, "PopBubbles", 8, popped_reads, elba_pop_bubbles, cfg);
}

// CutWeakOverlaps(S, myreads, min_ratio_q16) — not in the reference: elba_cut_weak_overlaps on the S that TransitiveReduction (or ClipTips, or
// PopBubbles) left on the device, before GenerateContigs.  Where an end of a read (direction & 1 of the column's entries) has two or more
// overlaps, those whose score * 65536 is below min_ratio_q16 times the best score of that end leave S, and so does every entry whose mirror
// image is such a one; in one pass.  Entries leave, no read does, and the read flags stay; the host copy of S is replaced by the cut graph.
inline elba_weak_stats CutWeakOverlaps(StringGraph &S, const DnaBuffer &myreads, int min_ratio_q16)
{
    elba_weak_cfg cfg{};
    cfg.min_ratio_q16 = min_ratio_q16;
    return detail::clean_call<elba_weak_stats>(S, myreads, "CutWeakOverlaps", 0, nullptr, elba_cut_weak_overlaps, cfg);
}

// CutBridges(S, myreads, max_bridge_reads, min_flank_reads) — the rule of asmtools/bridge_removal.py for chains: elba_cut_bridges on the S that
// TransitiveReduction (or one of the three calls above) left on the device, before GenerateContigs.  A chain of at most max_bridge_reads reads
// of degree 2 between two reads of degree exactly 3, each of whose other two edges leads into at least min_flank_reads reads of degree 2,
// leaves S, in one pass; the two end reads stay.  The host copy of S is replaced by the cut graph, and cut_reads, if given, receives the reads
// removed so far (flag bit 4 of elba_export_read_flags), ascending.
inline elba_bridge_stats CutBridges(StringGraph &S, const DnaBuffer &myreads, int max_bridge_reads, int min_flank_reads, std::vector<int64_t> *cut_reads = nullptr)
{
    elba_bridge_cfg cfg{};
    cfg.max_bridge_reads = max_bridge_reads; cfg.min_flank_reads = min_flank_reads;
    return detail::clean_call<elba_bridge_stats>(S, myreads, "CutBridges", 16, cut_reads, elba_cut_bridges, cfg);
}

// ResolveStars(S, myreads, rounds) — the rule of asmtools/star_resolution.py: elba_resolve_stars on the S that TransitiveReduction (or one of the
// four calls above) left on the device, before GenerateContigs.  A read of degree 3 whose three neighbours all have degree 2 is a centre; when
// exactly one pair of the three neighbours is a pair of R — the overlaps TransitiveReduction started from, after its prunes, which the device
// keeps — the neighbour in no such pair leaves S with its entries, in up to `rounds` rounds; the centre stays.  The script's second argument,
// the overlap graph, is not passed: it is the R of the TransitiveReduction call that made S.  The host copy of S is replaced by the resolved
// graph, and odd_arms, if given, receives the reads removed so far (flag bit 5 of elba_export_read_flags), ascending.
inline elba_star_stats ResolveStars(StringGraph &S, const DnaBuffer &myreads, int rounds = 1, std::vector<int64_t> *odd_arms = nullptr)
{
    elba_star_cfg cfg{};
    cfg.rounds = rounds;
    return detail::clean_call<elba_star_stats>(S, myreads, "ResolveStars", 32, odd_arms, elba_resolve_stars, cfg);
}

// PileupVector (include/PruneChimeras.hpp:11-26): here a read's coverage is held as the (start, depth) segments elba_export_pileup returns;
// the per-base vector of the reference is built from them on request.
class PileupVector {
public:
    int length = 0;
    std::vector<int> seg_start, seg_depth;      // maximal runs of equal depth, starts ascending from 0, the last ends at length
    std::tuple<int, int> trimmed{-1, -1};       // what elba_read_pileup computed: [beststart, bestend + 1) or (-1, -1)
    uint8_t flags = 0;                          // bit 0 unsupported, bit 1 split
    int Length() const { return length; }
    std::vector<int> pileup() const
    {
        std::vector<int> v((size_t)length, 0);
        for (size_t j = 0; j < seg_start.size(); ++j) {
            const int e = j + 1 < seg_start.size() ? seg_start[j + 1] : length;
            for (int i = seg_start[j]; i < e; ++i) v[(size_t)i] = seg_depth[j];
        }
        return v;
    }
    // GetTrimmedInterval (src/PruneChimeras.cpp:30-69) on the per-base vector, with the best run returned (the reference returns the run still
    // open at the last base) half-open; maxlen = the reference's starting 2500.  The host restatement the device's `trimmed` is held against.
    std::tuple<int, int> GetTrimmedInterval(int threshold, int maxlen = 2500) const
    {
        const std::vector<int> p = pileup();
        int beststart = -1, bestend = -1, start = -1, end = -1;
        double bestavg = 0;
        long long curbases = 0;
        for (int i = 0; i < length; ++i) {
            if (p[(size_t)i] >= threshold) {
                if (start == -1) { curbases = 0; start = i; }
                end = i;
                curbases += p[(size_t)i];
                const int span = end - start + 1;
                const double curavg = static_cast<double>(curbases) / static_cast<double>(span);
                if (span > maxlen && curavg > bestavg) { beststart = start; bestend = end; maxlen = span; bestavg = curavg; }
            } else {
                start = -1; end = -1;
            }
        }
        return beststart < 0 ? std::make_tuple(-1, -1) : std::make_tuple(beststart, bestend + 1);
    }
};

// GetReadPileup(dfd, Rmat) — src/PruneChimeras.cpp:108-158, on the symmetrised R (both reads of a pair credited; the reference credits only
// the column read of the upper triangle) and on the device: elba_read_pileup on the pairs the next TransitiveReduction reads.
inline std::vector<PileupVector> GetReadPileup(const DnaBuffer &myreads, OverlapMatrix &R, const elba_pileup_cfg &cfg, elba_pileup_stats *stats = nullptr)
{
    if ((int64_t)myreads.size() != R.numreads) throw Error(ELBA_ERR_INVALID_ARG, "GetReadPileup: myreads does not hold the overlaps' reads");
    if (!R.engine) throw Error(ELBA_ERR_STATE, "GetReadPileup: the overlaps are not on a device");
    elba_pileup_stats st{};
    R.engine->check(elba_read_pileup(R.engine->ctx, &cfg, &st));
    if (stats) *stats = st;
    elba_pileup_t o;
    R.engine->check(elba_export_pileup(R.engine->ctx, &o));
    std::vector<PileupVector> out((size_t)o.n);
    for (int64_t v = 0; v < o.n; ++v) {
        PileupVector &p = out[(size_t)v];
        p.length = (int)myreads.lengths()[v];
        p.seg_start.assign(o.seg_start + o.seg_off[v], o.seg_start + o.seg_off[v + 1]);
        p.seg_depth.assign(o.seg_depth + o.seg_off[v], o.seg_depth + o.seg_off[v + 1]);
        p.trimmed = std::make_tuple(o.trim_beg[v], o.trim_end[v]);
        p.flags = o.flags[v];
    }
    elba_free_pileup(&o);
    return out;
}

// R->PruneFull(x, x) for x = the reads with flags & mask (CombBLAS SpParMat::PruneFull): the kept pairs become the edge list the next
// TransitiveReduction reads; the host copy of R is pruned alike.  Returns the pairs kept.
inline int64_t PruneFull(OverlapMatrix &R, int mask)
{
    if (!R.engine) throw Error(ELBA_ERR_STATE, "PruneFull: the overlaps are not on a device");
    std::vector<uint8_t> flags;
    {
        elba_pileup_t o;
        R.engine->check(elba_export_pileup(R.engine->ctx, &o));
        flags.assign(o.flags, o.flags + o.n);
        elba_free_pileup(&o);
    }
    int64_t kept = 0;
    R.engine->check(elba_prune_reads(R.engine->ctx, mask, &kept));
    size_t w = 0;
    for (size_t a = 0; a < R.vals.size(); ++a) {
        if ((flags[(size_t)R.rows[a]] | flags[(size_t)R.cols[a]]) & mask) continue;
        R.rows[w] = R.rows[a]; R.cols[w] = R.cols[a]; R.vals[w] = R.vals[a]; ++w;
    }
    R.rows.resize(w); R.cols.resize(w); R.vals.resize(w);
    if ((int64_t)w != kept) throw Error(ELBA_ERR_INTERNAL, "PruneFull: the device kept " + std::to_string(kept) + " pairs, the host " + std::to_string(w));
    return kept;
}

// The reads cut to their supported intervals (elba_trim_reads): what GetTrimmedInterval's interval is computed for; the reference stops
// before this step.  TrimReads cuts the reads of the last GetReadPileup on the device — mode 0: every read to its trimmed interval, mode 1:
// one piece per long run, so that a chimera is split — and leaves the pieces there; ExportTrimMap says where each piece came from,
// TrimmedReadsDevice hands out their device addresses, AdoptTrimmedReads makes them the engine's reads (as after elba_set_reads) and returns
// them as the DnaBuffer the next get_kmer_count_map_keys(..., engine) round reads its lengths from.
struct TrimMap {
    std::vector<int64_t> src_read;              // piece p = bases [src_beg, src_end) of read src_read; (src_read, src_beg) ascending
    std::vector<int32_t> src_beg, src_end;
    size_t size() const { return src_read.size(); }
};

struct TrimmedReadsView { const void *d_packed = nullptr, *d_byte_off = nullptr, *d_len = nullptr; int64_t packed_bytes = 0, n = 0; };

inline elba_trim_stats TrimReads(OverlapMatrix &R, const elba_trim_cfg &cfg)
{
    if (!R.engine) throw Error(ELBA_ERR_STATE, "TrimReads: the overlaps are not on a device");
    elba_trim_stats st{};
    R.engine->check(elba_trim_reads(R.engine->ctx, &cfg, &st));
    return st;
}

inline TrimMap ExportTrimMap(OverlapMatrix &R)
{
    if (!R.engine) throw Error(ELBA_ERR_STATE, "ExportTrimMap: the overlaps are not on a device");
    elba_trim_map_t m;
    R.engine->check(elba_export_trim_map(R.engine->ctx, &m));
    TrimMap out;
    out.src_read.assign(m.src_read, m.src_read + m.n); out.src_beg.assign(m.src_beg, m.src_beg + m.n); out.src_end.assign(m.src_end, m.src_end + m.n);
    elba_free_trim_map(&m);
    return out;
}

inline TrimmedReadsView TrimmedReadsDevice(OverlapMatrix &R)
{
    if (!R.engine) throw Error(ELBA_ERR_STATE, "TrimmedReadsDevice: the overlaps are not on a device");
    TrimmedReadsView v;
    R.engine->check(elba_get_trimmed_reads_device(R.engine->ctx, &v.d_packed, &v.packed_bytes, &v.d_byte_off, &v.d_len, &v.n));
    return v;
}

// R's engine holds the pieces afterwards and nothing derived from the old reads: R itself (the host triples) describes the old reads.
inline DnaBuffer AdoptTrimmedReads(OverlapMatrix &R)
{
    const TrimmedReadsView v = TrimmedReadsDevice(R);
    R.engine->check(elba_adopt_trimmed_reads(R.engine->ctx));
    std::vector<uint8_t> buf((size_t)v.packed_bytes);
    std::vector<uint64_t> off((size_t)v.n);
    std::vector<uint32_t> len((size_t)v.n);
    R.engine->check(elba_export_reads(R.engine->ctx, buf.data(), v.packed_bytes, off.data(), len.data(), v.n));
    return DnaBuffer::from_packed(std::move(buf), std::move(off), std::move(len));
}

// GenerateContigs(S, mydna, dfd) — src/ContigGeneration.cpp:376-457 on one rank: branches (degree > 2) dropped, every path of >= 2 reads
// walked from its smaller-id end, the contig built from the reads' prefixes; on the GPU, on the S that TransitiveReduction left there.
// The reads are the ones the context was given (mydna on one rank).  Contigs in the reference's emission order.
// flags (not in the reference): ELBA_CONTIG_CIRCULAR also walks every cycle once round from its smallest read, ELBA_CONTIG_SINGLETONS also
// emits every unflagged read outside all paths and cycles as a contig of its own; contigs of all kinds by ascending start read.  kinds, if
// given, receives one byte per contig: 0 path, 1 circular, 2 single read.
inline std::vector<std::string> GenerateContigs(StringGraph &S, const DnaBuffer &mydna, elba_contig_stats *stats = nullptr, int flags = 0,
                                                std::vector<uint8_t> *kinds = nullptr)
{
    if (!S.engine) throw Error(ELBA_ERR_STATE, "GenerateContigs: the string graph is not on a device");
    if ((int64_t)mydna.size() != S.numreads) throw Error(ELBA_ERR_INVALID_ARG, "GenerateContigs: mydna does not hold the graph's reads");
    elba_contig_stats st{};
    elba_contig_cfg cfg{};
    cfg.flags = flags;
    S.engine->check(elba_generate_contigs_ex(S.engine->ctx, &cfg, &st));
    if (stats) *stats = st;
    elba_contigs_t c;
    S.engine->check(elba_export_contigs(S.engine->ctx, &c));
    std::vector<std::string> contigs;
    contigs.reserve((size_t)c.n);
    for (int64_t i = 0; i < c.n; ++i) contigs.emplace_back(c.seq + c.seq_off[i], (size_t)(c.seq_off[i + 1] - c.seq_off[i]));
    elba_free_contigs(&c);
    if (kinds) {
        kinds->assign(contigs.size(), 0);
        S.engine->check(elba_export_contig_kinds(S.engine->ctx, kinds->data(), (int64_t)contigs.size()));
    }
    return contigs;
}

// parallel_write_contigs (src/main.cpp:487-512) on one rank: the Exscan offset is 0; the reference takes the name from
// get_contigs_fasta_name() (<prefix>.contigs.fa), here it is an argument.
// With kinds (GenerateContigs' own, one per contig) the header of a circular contig is `>contig<i> circular`; nothing else changes.
inline void parallel_write_contigs(const std::vector<std::string> &contigs, const std::string &contigs_fname, const std::vector<uint8_t> *kinds = nullptr)
{
    if (kinds && kinds->size() != contigs.size()) throw Error(ELBA_ERR_INVALID_ARG, "parallel_write_contigs: one kind per contig");
    std::stringstream contig_filecontents;
    for (size_t i = 0; i < contigs.size(); ++i)
        contig_filecontents << ">contig" << i << (kinds && (*kinds)[i] == 1 ? " circular" : "") << "\n" << contigs[i] << "\n";
    std::ofstream f(contigs_fname, std::ios::binary);
    const std::string cfs = contig_filecontents.str();
    f.write(cfs.data(), (std::streamsize)cfs.size());
    if (!f) throw Error(ELBA_ERR_INVALID_ARG, "parallel_write_contigs: cannot write " + contigs_fname);
}

// assembly_links(S) — elba_export_assembly_links on the S and the contigs of the last GenerateContigs (the rule is stated in
// include/elba_amd.h): the edges of S at branch reads as links between contig ends, one closure record per circular contig, sorted by
// (from_read, to_read).  An export: S and the contigs stay as they are.
inline std::vector<elba_link_t> assembly_links(StringGraph &S, elba_graph_stats *stats = nullptr)
{
    if (!S.engine) throw Error(ELBA_ERR_STATE, "assembly_links: the string graph is not on a device");
    elba_links_t l;
    elba_graph_stats st{};
    S.engine->check(elba_export_assembly_links(S.engine->ctx, &l, &st));
    std::vector<elba_link_t> links(l.links, l.links + l.n);
    elba_free_links(&l);
    if (stats) *stats = st;
    return links;
}

// write_gfa — GFA 1, byte for byte what formats.write_gfa writes: `H\tVN:Z:1.0`, one `S\tcontig<i>\t<seq>\tLN:i:<len>` per contig (the names
// of parallel_write_contigs; with chain_reads, the reads per contig, also `\tRC:i:<reads>`) and one `L\tcontig<a>\t+|-\tcontig<b>\t+|-\t<overlap>M`
// per record, closures included.  kinds, if given, is checked against the closures: one per circular contig.  With depth, the credited
// bases per contig (Placements::credited_bases), every S line also ends in `\tDP:f:<credited bases / length>` with two decimals.
inline void write_gfa(const std::string &gfa_fname, const std::vector<std::string> &contigs, const std::vector<uint8_t> *kinds, const std::vector<elba_link_t> &links,
                      const std::vector<int64_t> *chain_reads = nullptr, const std::vector<int64_t> *depth = nullptr)
{
    const size_t n = contigs.size();
    if (kinds && kinds->size() != n) throw Error(ELBA_ERR_INVALID_ARG, "write_gfa: one kind per contig");
    if (chain_reads && chain_reads->size() != n) throw Error(ELBA_ERR_INVALID_ARG, "write_gfa: one read count per contig");
    if (depth && depth->size() != n) throw Error(ELBA_ERR_INVALID_ARG, "write_gfa: one depth (credited bases) per contig");
    if (kinds) {
        std::vector<uint32_t> closed, circular;
        for (const elba_link_t &r : links) if (r.flags & 1) closed.push_back(r.from);
        std::sort(closed.begin(), closed.end());
        for (size_t i = 0; i < n; ++i) if ((*kinds)[i] == 1) circular.push_back((uint32_t)i);
        if (closed != circular) throw Error(ELBA_ERR_INVALID_ARG, "write_gfa: the closure records are not those of the circular contigs");
    }
    std::stringstream out;
    out << "H\tVN:Z:1.0\n";
    for (size_t i = 0; i < n; ++i) {
        out << "S\tcontig" << i << "\t" << contigs[i] << "\tLN:i:" << contigs[i].size();
        if (chain_reads) out << "\tRC:i:" << (*chain_reads)[i];
        if (depth) {
            char dp[64];
            std::snprintf(dp, sizeof(dp), "\tDP:f:%.2f", contigs[i].empty() ? 0.0 : (double)(*depth)[i] / (double)contigs[i].size());
            out << dp;
        }
        out << "\n";
    }
    for (const elba_link_t &r : links) {
        if (r.from >= n || r.to >= n) throw Error(ELBA_ERR_INVALID_ARG, "write_gfa: a link names a contig that is not there");
        out << "L\tcontig" << r.from << "\t" << (r.from_rev ? "-" : "+") << "\tcontig" << r.to << "\t" << (r.to_rev ? "-" : "+") << "\t" << r.overlap << "M\n";
    }
    std::ofstream f(gfa_fname, std::ios::binary);
    const std::string text = out.str();
    f.write(text.data(), (std::streamsize)text.size());
    if (!f) throw Error(ELBA_ERR_INVALID_ARG, "write_gfa: cannot write " + gfa_fname);
}

// graph_components(S, graph) — elba_graph_components on the engine of S (the rule is stated in include/elba_amd.h): the connected
// components of the string graph (ELBA_CC_STRING) or of the passed pairs it was built from (ELBA_CC_OVERLAPS), every read in one,
// numbered by ascending smallest read, with the per-component counts.  An export: nothing on the engine changes.
struct Components {
    std::vector<int32_t> comp_of_read;                                       // one per read of the graph
    std::vector<int64_t> first_read, reads, bases, edges, branches, ends;    // per component
};

inline Components graph_components(StringGraph &S, int graph = ELBA_CC_STRING, bool bases = false, elba_cc_stats *stats = nullptr)
{
    if (!S.engine) throw Error(ELBA_ERR_STATE, "graph_components: the string graph is not on a device");
    elba_cc_cfg cfg{};
    cfg.graph = graph; cfg.flags = bases ? ELBA_CC_BASES : 0;
    elba_components_t o;
    elba_cc_stats st{};
    S.engine->check(elba_graph_components(S.engine->ctx, &cfg, &o, &st));
    Components c;
    try {
        c.comp_of_read.assign(o.comp_of_read, o.comp_of_read + o.nreads);
        c.first_read.assign(o.first_read, o.first_read + o.n); c.reads.assign(o.reads, o.reads + o.n); c.bases.assign(o.bases, o.bases + o.n);
        c.edges.assign(o.edges, o.edges + o.n); c.branches.assign(o.branches, o.branches + o.n); c.ends.assign(o.ends, o.ends + o.n);
    } catch (...) {
        elba_free_components(&o);
        throw;
    }
    elba_free_components(&o);
    if (stats) *stats = st;
    return c;
}

// partition_components(S, nparts) — elba_partition_components: the components of at least min_reads reads dealt to nparts parts, heaviest
// first, each to the part with the smallest sum so far (the reference's GetLocalProcAssignments, ties closed).  part_of_read: one per
// read, -1 for a read of a smaller component; part_weight: the sums.  A multi-GPU driver hands part p's reads to rank p.
struct Partition {
    std::vector<int32_t> part_of_read;
    std::vector<int64_t> part_weight;
};

inline Partition partition_components(StringGraph &S, int nparts, int graph = ELBA_CC_STRING, int weight = 0, int min_reads = 2)
{
    if (!S.engine) throw Error(ELBA_ERR_STATE, "partition_components: the string graph is not on a device");
    elba_part_cfg cfg{};
    cfg.graph = graph; cfg.nparts = nparts; cfg.weight = weight; cfg.min_reads = min_reads;
    Partition p;
    p.part_of_read.assign((size_t)S.numreads, -1);
    p.part_weight.assign((size_t)(nparts > 0 ? nparts : 1), 0);
    S.engine->check(elba_partition_components(S.engine->ctx, &cfg, p.part_of_read.data(), S.numreads, p.part_weight.data()));
    p.part_weight.resize((size_t)(nparts > 0 ? nparts : 0));
    return p;
}

// induce_part(engine, part_of_read, part) — elba_induce_part (the rule and the guarantee are stated in include/elba_amd.h): the reference's
// GetInducedReadSequences + ImposeMyReadDistribution for one part.  The reads v of the graph's input with part_of_read[v] == part,
// renumbered in order, as a DnaBuffer; the pairs between them; and per new read the pairs that leave the part, which load_part hands to
// the engine that assembles the part so that its bad reads are the whole run's.  An export: nothing on the engine changes.
struct InducedPart {
    std::vector<int64_t> old_of_new;                                          // new read -> read of the whole input, ascending
    DnaBuffer reads;                                                          // (empty without bases)
    bool has_reads = false;
    std::vector<int64_t> rows, cols;
    std::vector<elba_overlap_t> vals;
    std::vector<uint32_t> outside_aligned, outside_passed;                    // per new read
    elba_induce_stats stats{};
    int64_t numreads() const { return (int64_t)old_of_new.size(); }
};

inline InducedPart induce_part(detail::Engine &engine, const std::vector<int32_t> &part_of_read, int part, bool bases = true)
{
    elba_induce_cfg cfg{};
    cfg.part = part; cfg.flags = ELBA_INDUCE_HOST | (bases ? ELBA_INDUCE_BASES : 0);
    const int32_t none = 0;
    elba_induced_t o;
    InducedPart p;
    engine.check(elba_induce_part(engine.ctx, &cfg, part_of_read.empty() ? &none : part_of_read.data(), (int64_t)part_of_read.size(), &o, &p.stats));
    try {
        p.old_of_new.assign(o.old_of_new, o.old_of_new + o.reads);
        p.rows.assign(o.rows, o.rows + o.pairs); p.cols.assign(o.cols, o.cols + o.pairs); p.vals.assign(o.vals, o.vals + o.pairs);
        p.outside_aligned.assign(o.outside_aligned, o.outside_aligned + o.reads); p.outside_passed.assign(o.outside_passed, o.outside_passed + o.reads);
        if (bases) {
            p.reads = DnaBuffer::from_packed(std::vector<uint8_t>(o.packed, o.packed + o.packed_bytes + 16), std::vector<uint64_t>(o.byte_off, o.byte_off + o.reads),
                                             std::vector<uint32_t>(o.len, o.len + o.reads));
            p.has_reads = true;
        }
    } catch (...) {
        elba_free_induced(&o);
        throw;
    }
    elba_free_induced(&o);
    return p;
}

// load_part(engine, p) — the part becomes the input of `engine`: elba_set_reads (when the part carries bases), elba_set_overlaps and
// elba_set_outside_counts.  outside = false leaves the counts out: what a driver without them computes (no guarantee).
inline void load_part(detail::Engine &engine, const InducedPart &p, bool outside = true)
{
    const int64_t R = p.numreads();
    if (p.has_reads) engine.check(elba_set_reads(engine.ctx, p.reads.data(), p.reads.offsets(), p.reads.lengths(), R, 0));
    engine.check(elba_set_overlaps(engine.ctx, R, p.rows.data(), p.cols.data(), p.vals.data(), (int64_t)p.rows.size()));
    const uint32_t none = 0;                                                  // (null arrays would detach)
    if (outside) engine.check(elba_set_outside_counts(engine.ctx, R, R ? p.outside_aligned.data() : &none, R ? p.outside_passed.data() : &none));
}

// place_reads(S) — elba_place_reads on the S, the contigs of the last GenerateContigs and the pairs S was built from (the rule is stated in
// include/elba_amd.h): every read on its contig — chain reads where the contig stage put them, the others through their best passed pair
// with a chain read — and per contig the runs of equal depth and the credits.  An export: nothing on the engine changes.
struct Placements {
    std::vector<elba_placement_t> reads;                        // one per read of the graph
    std::vector<int64_t> seg_off;                               // [contigs + 1] into the two below
    std::vector<int32_t> seg_start, seg_depth;
    std::vector<int64_t> credited_reads, credited_bases;        // per contig
};

inline Placements place_reads(StringGraph &S, int skip_flags = 1, elba_place_stats *stats = nullptr)
{
    if (!S.engine) throw Error(ELBA_ERR_STATE, "place_reads: the string graph is not on a device");
    elba_place_cfg cfg{};
    cfg.skip_flags = skip_flags;
    elba_placements_t o;
    elba_place_stats st{};
    S.engine->check(elba_place_reads(S.engine->ctx, &cfg, &o, &st));
    Placements p;
    try {
        const int64_t nseg = o.seg_off[o.ncontigs];
        p.reads.assign(o.reads, o.reads + o.nreads); p.seg_off.assign(o.seg_off, o.seg_off + o.ncontigs + 1);
        p.seg_start.assign(o.seg_start, o.seg_start + nseg); p.seg_depth.assign(o.seg_depth, o.seg_depth + nseg);
        p.credited_reads.assign(o.credited_reads, o.credited_reads + o.ncontigs); p.credited_bases.assign(o.credited_bases, o.credited_bases + o.ncontigs);
    } catch (...) {
        elba_free_placements(&o);
        throw;
    }
    elba_free_placements(&o);
    if (stats) *stats = st;
    return p;
}

// polish_contigs(S) — elba_polish_contigs on the S, the contigs of the last GenerateContigs, the reads and the pairs S was built from (the
// rule is stated in include/elba_amd.h): every placed read aligned to its stretch of its contig in a band, the alignments voting per column
// and gap, the contigs the votes call.  An export: nothing on the engine changes.  votes: also the counts per column and gap and the
// per-read records.  The polished contigs are written like the others (write_contigs_fasta, write_gfa).
struct Polished {
    std::vector<std::string> contigs;                           // the order of GenerateContigs
    std::vector<int64_t> voters, substituted, deleted, inserted;      // per contig
    std::vector<int64_t> col_off;                               // votes only: [contigs + 1], the offsets of the unpolished contigs
    std::vector<uint32_t> col, gap;                             // 5 per column; 4 per gap, contig k's gap g at 4 * (col_off[k] + k + g)
    std::vector<elba_polish_read_t> reads;                      // one per read of the graph
};

inline Polished polish_contigs(StringGraph &S, int skip_flags = 1, int band = 64, double max_diff = 0.25, int min_depth = 3, bool votes = false, elba_polish_stats *stats = nullptr)
{
    if (!S.engine) throw Error(ELBA_ERR_STATE, "polish_contigs: the string graph is not on a device");
    elba_polish_cfg cfg{};
    cfg.skip_flags = skip_flags; cfg.band = band; cfg.max_diff_q16 = (int32_t)(max_diff * 65536.0 + 0.5); cfg.min_depth = min_depth; cfg.flags = votes ? ELBA_POLISH_EXPORT_VOTES : 0;
    elba_polished_t o;
    elba_polish_stats st{};
    S.engine->check(elba_polish_contigs(S.engine->ctx, &cfg, &o, &st));
    Polished p;
    try {
        for (int64_t i = 0; i < o.n; ++i) p.contigs.emplace_back(o.seq + o.seq_off[i], (size_t)(o.seq_off[i + 1] - o.seq_off[i]));
        p.voters.assign(o.voters, o.voters + o.n); p.substituted.assign(o.substituted, o.substituted + o.n);
        p.deleted.assign(o.deleted, o.deleted + o.n); p.inserted.assign(o.inserted, o.inserted + o.n);
        if (votes) {
            const int64_t bases = o.col_off[o.n];
            p.col_off.assign(o.col_off, o.col_off + o.n + 1); p.col.assign(o.col, o.col + 5 * bases); p.gap.assign(o.gap, o.gap + 4 * (bases + o.n));
            p.reads.assign(o.reads, o.reads + o.nreads);
        }
    } catch (...) {
        elba_free_polished(&o);
        throw;
    }
    elba_free_polished(&o);
    if (stats) *stats = st;
    return p;
}

// write_placements_paf — byte for byte what formats.write_placements_paf writes: one line per placed read, by ascending read — name, length,
// the credited interval in forward read coordinates, strand, `contig<i>`, its length, the target interval, the anchor pair's score, the
// block length and 255.  On a path or single-read contig the target interval is [max(start, 0), min(start + len, L)), empty at the nearer
// end for a read outside; on a circular contig min(len, L) bases from start mod L, the end of a wrapped read running past L (a reader that
// wants tend <= tlen splits such a line at L).  kinds says which contigs are circular; without it none may be: a wrapped record throws.
inline void write_placements_paf(const std::string &paf_fname, const Placements &pl, const std::vector<std::string> &names, const std::vector<int64_t> &lens,
                                 const std::vector<int64_t> &contig_lens, const std::vector<uint8_t> *kinds = nullptr)
{
    if (pl.reads.size() != names.size() || names.size() != lens.size()) throw Error(ELBA_ERR_INVALID_ARG, "write_placements_paf: one record, one name and one length per read");
    if (kinds && kinds->size() != contig_lens.size()) throw Error(ELBA_ERR_INVALID_ARG, "write_placements_paf: one kind per contig");
    std::stringstream out;
    for (size_t r = 0; r < pl.reads.size(); ++r) {
        const elba_placement_t &p = pl.reads[r];
        if (!p.kind) continue;
        if (p.contig < 0 || (size_t)p.contig >= contig_lens.size()) throw Error(ELBA_ERR_INVALID_ARG, "write_placements_paf: a read names a contig that is not there");
        if (!kinds && (p.flags & 4)) throw Error(ELBA_ERR_INVALID_ARG, "write_placements_paf: a wrapped read lies on a circular contig: give the contigs' kinds");
        const int64_t start = p.start, l = lens[r], L = contig_lens[(size_t)p.contig];
        int64_t tb, te, ob, oe;
        if (kinds && (*kinds)[(size_t)p.contig] == 1) {
            const int64_t cred = std::min(l, L);
            tb = L > 0 ? ((start % L) + L) % L : 0;
            te = tb + cred; ob = 0; oe = cred;
        } else {
            tb = std::min(std::max<int64_t>(start, 0), L);
            te = std::max(tb, std::min(start + l, L));
            ob = std::min(std::max<int64_t>(tb - start, 0), l); oe = std::min(std::max<int64_t>(te - start, 0), l);
        }
        const int64_t qb = p.strand ? l - oe : ob, qe = p.strand ? l - ob : oe;
        out << names[r] << "\t" << l << "\t" << qb << "\t" << qe << "\t" << (p.strand ? "-" : "+") << "\tcontig" << p.contig << "\t" << L << "\t" << tb << "\t" << te << "\t"
            << p.score << "\t" << te - tb << "\t255\n";
    }
    std::ofstream f(paf_fname, std::ios::binary);
    const std::string text = out.str();
    f.write(text.data(), (std::streamsize)text.size());
    if (!f) throw Error(ELBA_ERR_INVALID_ARG, "write_placements_paf: cannot write " + paf_fname);
}

// ---- the reference's text outputs -------------------------------------------------------------------------------
// SharedSeeds as operator<< prints it (include/SharedSeeds.hpp:75-88): `{(q0,t0),(q1,t1),n}` with min(numshared, 2) seeds.
inline std::ostream &operator<<(std::ostream &os, const SharedSeeds &o)
{
    const int seedstoprint = o.getnumstored() < 2 ? o.getnumstored() : 2;
    os << "{";
    for (int i = 0; i < seedstoprint; ++i) os << "(" << std::get<0>(o.seeds[i]) << "," << std::get<1>(o.seeds[i]) << "),";
    os << o.getnumshared() << "}";
    return os;
}

// Overlap as operator<< prints it (include/Overlap.hpp:78-83)
inline std::ostream &operator<<(std::ostream &os, const Overlap &o)
{
    os << std::get<0>(o.len) << "\t" << std::get<0>(o.beg) << "\t" << std::get<0>(o.end) << "\t" << (o.rc ? '-' : '+') << "\t" << std::get<1>(o.len) << "\t" << std::get<1>(o.beg) << "\t"
       << std::get<1>(o.end) << "\t" << o.score << "\t" << static_cast<int>(o.direction) << "\t" << static_cast<int>(o.suffix);
    return os;
}

// ELBALogger::log_seed_matrix (src/ELBALogger.cpp:22-35): B.ParallelWriteMM("B.mtx", true, SharedSeeds::IOHandler()) — MatrixMarket
// coordinate file, one-based indices, entries as the local DCSC stores them (column by column, rows ascending), values through
// IOHandler::save = operator<<.  (CombBLAS's writer itself is un-vendored: the header line follows the MatrixMarket convention.)
inline void log_seed_matrix(SeedMatrix &B, const std::string &fname)
{
    std::ofstream os(fname);
    if (!os) throw Error(ELBA_ERR_INVALID_ARG, "cannot open " + fname);
    const SeqSeedMatrix *seq = B.seqptr();
    const Dcsc *dcsc = seq->GetDCSC();
    os << "%%MatrixMarket matrix coordinate real general\n" << B.getnrow() << " " << B.getncol() << " " << seq->getnnz() << "\n";
    if (dcsc)
        for (int64_t i = 0; i < dcsc->nzc; ++i)
            for (int64_t j = dcsc->cp[(size_t)i]; j < dcsc->cp[(size_t)i + 1]; ++j) os << dcsc->ir[(size_t)j] + 1 << "\t" << dcsc->jc[(size_t)i] + 1 << "\t" << dcsc->numx[(size_t)j] << "\n";
}

// parallel_write_paf (src/main.cpp:514-551) for the triples of R or S: the reference walks the local DCSC (columns ascending, rows ascending
// within a column) and prints `maplen` as written there (:536: max(endQ - begQ, endT - endT)).
namespace detail {
template <class M>
inline void write_paf(const M &R, const std::vector<std::string> &names, const std::string &pafname)
{
    std::vector<size_t> order(R.vals.size());
    for (size_t a = 0; a < order.size(); ++a) order[a] = a;
    std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return R.cols[x] != R.cols[y] ? R.cols[x] < R.cols[y] : R.rows[x] < R.rows[y]; });
    std::ofstream ss(pafname);
    if (!ss) throw Error(ELBA_ERR_INVALID_ARG, "cannot open " + pafname);
    for (size_t a : order) {
        const Overlap &o = R.vals[a];
        const long long begQ = std::get<0>(o.beg), endQ = std::get<0>(o.end), endT = std::get<1>(o.end);
        const long long maplen = std::max(endQ - begQ, endT - endT);
        ss << names[(size_t)R.rows[a]] << "\t" << std::get<0>(o.len) << "\t" << std::get<0>(o.beg) << "\t" << std::get<0>(o.end) << "\t" << "+-"[o.rc ? 1 : 0] << "\t"
           << names[(size_t)R.cols[a]] << "\t" << std::get<1>(o.len) << "\t" << std::get<1>(o.beg) << "\t" << std::get<1>(o.end) << "\t" << o.score << "\t" << maplen << "\t255\t"
           << static_cast<int>(o.passed) << "\n";
    }
}
}  // namespace detail
inline void parallel_write_paf(const OverlapMatrix &R, const std::vector<std::string> &names, const std::string &pafname) { detail::write_paf(R, names, pafname); }
inline void parallel_write_paf(const StringGraph &S, const std::vector<std::string> &names, const std::string &pafname) { detail::write_paf(S, names, pafname); }

}  // namespace elba
