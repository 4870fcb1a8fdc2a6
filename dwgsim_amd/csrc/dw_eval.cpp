// dw_eval.cpp -- host side of dwgsim_eval-hip: the dwgsim_hip_eval_* C-ABI (include/dwgsim_hip.h), chunking of the SAM text, the @SQ tables,
// and the reference's output text (dwgsim_eval.c dwgsim_eval_counts_print / dwgsim_eval_print_error).
//
// Chunks.  Two slots, each a page-locked text buffer and its device buffers on a stream of its own.  The caller's bytes are copied into the
// filling slot; when it is full, the text up to its last newline is submitted (copy up, four kernels, copy back the per-chunk result) and the
// other slot becomes the filling one: it starts with the last line of the submitted chunk (the context line that -m compares the next record
// with) and the partial line that did not fit.  So the copy and the kernels of one chunk overlap with the host filling the next.  Results are
// read back in submission order: the first chunk with a fatal record ends the run, and its record is the first one in file order.
//
// BAM files (bam_begin / feed_bam).  The caller's compressed bytes are collected; every complete BGZF block (dw_bam.hpp) becomes a job whose
// destination in the filling slot follows from the ISIZE of the blocks in front of it, and the jobs of one feed are inflated in place by the
// worker threads (dw_inflate.hpp; CRC-32 and ISIZE checked per block).  The calling thread then hops over the block_size chain of the new
// bytes and notes the offset of every whole record.  A slot that cannot take the next block is cut after its last whole record and submitted:
// text and offsets up, k_eval_bam_records, result back; the other slot continues with that last record as context and the partial record
// behind it.  The first blocks of a file are inflated aside until the BAM header is complete; its reference list becomes the targets.
// Breakdown (set_breakdown; dw_eval.hpp BREAKDOWN).  The same chunks go through the breakdown form of the record kernel, which counts into the
// strata of the selected dimensions (dw_eval_launch.hpp EvalBdArgs) instead of the one histogram.  finish() makes the main table from the sum of
// the first selected dimension's strata and one section per stratum; tables, sections and the dimension list are dw_eval_table.hpp's.
// Truth (truth_header / truth_feed / truth_commit; dw_eval.hpp TRUTH).  Before the first file, truth text fills slot 0; every full slot is cut at
// its last newline and loaded (truth_chunk: newline kernels, count, scan, write -- each step sized by what the one before produced), commit
// builds the index and checks it.  With a committed truth the chunks go through the truth form of the record kernel, and every header /
// bam_begin uploads the map from the file's targets to the truth's contigs (map_contigs).  finish() makes the section from the 64-bit counters.
// A container error (framing, inflate, CRC, ISIZE, magic, header, a file that ends inside something) first evaluates the whole records in
// front of it: a fatal record there wins; otherwise the call returns DWGSIM_HIP_ERR_FAILED and last_error says what and where.
//
// The file in order.  The context's parts, each a struct: Slot and Pipeline (the chunks), NameTable (the targets of the current file; the
// truth's contigs), BamStream, Outcome (what finish() reports), BreakdownRun, TruthRun.  Then: the kernels' arguments and launch(), the one
// place that knows the run's form; process_oldest / hand_over / submit, the one way a chunk of either format goes to the device and comes
// back; end_file; the name tables' upload; the BAM stream (whole_record, hop_records, bam_pump); convert_ctx; the truth's load; the texts;
// begin_file, what header and bam_begin share; the C-ABI.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdio.h>
#include <string.h>
#include <time.h>
#include <algorithm>
#include <array>
#include <deque>
#include <map>
#include <memory>
#include <string>
#include <utility>
#include <vector>
#include "dw_bam.hpp"
#include "dw_eval_launch.hpp"
#include "dw_eval_table.hpp"
#include "dw_mem.hpp"
#include "../../include/dwgsim_hip.h"

using namespace dw;

namespace {

constexpr size_t DEFAULT_CHUNK = 32ull << 20, MIN_CHUNK = 4096, MAX_CHUNK = 1ull << 30;
constexpr int32_t WIN_LO = -EVAL_WIN / 2;
constexpr int DEFAULT_INFLATE_THREADS = 8, MAX_INFLATE_THREADS = 16;
constexpr size_t MAX_BATCH = 4096;      // BGZF blocks per inflate_blocks call
enum { FMT_SAM = 0, FMT_BAM = 1 };
const char BREAK_LINE[] = "************************************************************\n";

struct Slot {
    HostMem h_text, h_res, h_offs;      // page-locked: the text (its capacity is the slot's), an EvalRes, the record offsets of a BAM chunk
    DevMem d_text, d_ends, d_tiles, d_res, d_spill, d_flags;      // text, u32, u32, EvalRes, u64, u8
    DevStream st;               // (dwgsim_hip_eval_destroy waits for it before the context goes: the order in which the members then go does not matter)
    DevEvent e0, e1;
    size_t fill = 0, ctx_len = 0, len = 0;
    uint32_t has_ctx = 0;
    bool busy = false;
    int fmt = FMT_SAM;          // of the context record and what follows it
    uint32_t n_offs = 0;        // BAM: whole records found so far (the context record is the first), and where the next one starts
    size_t hop = 0;
};

// The chunk pipeline: the filling slot s[cur], and the submitted ones in submission order.
struct Pipeline {
    Slot s[2];
    int cur = 0;
    std::deque<int> pending;
    Slot &filling() { return s[cur]; }
};

// A name table: contig names, names[off[t] .. off[t + 1]), with the open-addressing hash of ev::Targets over them (a repeated name: the first);
// host copies (messages, map_contigs) and device copies (kernels).  tg is over the device copies, and empty until upload_names.
struct NameTable {
    std::string names;
    std::vector<uint32_t> off = {0};
    std::vector<int32_t> hash;
    DevMem d_names, d_off, d_hash;      // char, u32, i32
    ev::Targets tg = {};

    int32_t n() const { return (int32_t)off.size() - 1; }
    ev::Targets host() const { return {names.data(), off.data(), hash.data(), n(), (uint32_t)hash.size() - 1}; }

    // from a finished names / off pair (the reference list of a BAM header)
    void from_names(const std::string &nm, const std::vector<uint32_t> &o)
    {
        names = nm;
        off = o;
        uint32_t hs = 2;
        while (hs < 2u * (uint32_t)n()) hs <<= 1;
        hash.assign(hs, -1);
        for (int32_t t = 0; t < n(); ++t) {
            const uint32_t b = off[t], len = off[t + 1] - b;
            uint32_t h = ev::fnv1a(names.data() + b, len) & (hs - 1);
            while (hash[h] >= 0) {
                const int32_t u = hash[h];
                if (off[u + 1] - off[u] == len && !memcmp(names.data() + off[u], names.data() + b, len)) break;
                h = (h + 1) & (hs - 1);
            }
            if (hash[h] < 0) hash[h] = t;
        }
    }

    // from the SN: names of the @SQ lines of a header text
    void from_sq(const char *text, size_t len)
    {
        std::string nm;
        std::vector<uint32_t> o(1, 0);
        for (size_t p = 0; p < len;) {
            const char *nl = (const char *)memchr(text + p, '\n', len - p);
            const size_t e = nl ? (size_t)(nl - text) : len;
            if (e - p >= 3 && !memcmp(text + p, "@SQ", 3)) {
                for (size_t f = p; f < e;) {
                    const char *tab = (const char *)memchr(text + f, '\t', e - f);
                    const size_t fe = tab ? (size_t)(tab - text) : e;
                    if (f > p && fe - f >= 3 && !memcmp(text + f, "SN:", 3)) {
                        nm.append(text + f + 3, fe - f - 3);
                        o.push_back((uint32_t)nm.size());
                        break;
                    }
                    f = fe + 1;
                }
            }
            p = e + 1;
        }
        from_names(nm, o);
    }

    void drop_device()
    {
        d_names.reset(); d_off.reset(); d_hash.reset();
        tg = ev::Targets{};
    }
};

// The BGZF stream of the current BAM file, and what inflates it.
struct BamStream {
    int inflate_threads = DEFAULT_INFLATE_THREADS;
    std::unique_ptr<bam::InflatePool> pool;     // (made at the first use)
    std::vector<uint8_t> zbuf;          // compressed bytes not yet consumed: zbuf[zhead] is byte zpos of the file
    size_t zhead = 0;
    uint64_t zpos = 0;
    bool in_header = false;             // the BAM header is not complete yet
    bool bam_stop = false;              // a block_size that no record can have ended the stream
    std::vector<uint8_t> hdr_bytes;     // inflated bytes while the header is incomplete
    bam::Header bh;
    std::vector<bam::InflateJob> jobs;

    // the stream of a new file; the workers stay
    void restart()
    {
        BamStream fresh;
        fresh.inflate_threads = inflate_threads;
        fresh.pool = std::move(pool);
        fresh.in_header = true;
        *this = std::move(fresh);
    }
};

// The run's outcome: what finish() reports.  After the first fatal record (failed) nothing else is counted any more.
struct Outcome {
    bool failed = false;
    int code = 0;
    uint64_t err_rec = 0;
    std::string err_line;
    uint64_t n = 0, records = 0;
    std::string incorrect, table, stderr_text;
};

// The breakdown: what is selected, its device counters, its part of the spill lists, its text.
struct BreakdownRun {
    evt::Breakdown b;
    evt::BreakdownCounts spill;
    DevMem d_hist;                      // unsigned long long
    std::string text;
};

// The truth (dw_eval.hpp TRUTH): its contigs, its records, CIGAR pool and index on the device, the 64-bit counters, its text.
struct TruthRun {
    bool begun = false, fed = false, committed = false, bad = false;
    NameTable contigs;                  // (their device copies are the load's own, as d_cnt and d_err are: freed by commit)
    DevMem d_cnt, d_err;
    DevMem d_recs, d_pool, d_slots, d_ctrs, d_tmap;     // TruthRec, u32, u64, u64, i32
    uint64_t n_recs = 0, n_pool = 0;
    uint32_t mask = 0;
    int force_log2 = -1;
    std::string text;
};

} // namespace

// The fields outside the parts are the run's: options, state of the calls, the plain form's counters.  While fmt == FMT_SAM nothing of `bam`
// means anything but its workers; `bd` is empty unless bd.b.on, and `tr` unless tr.begun.
struct dwgsim_hip_eval_ctx {
    dwgsim_hip_eval_opts_t o;
    std::string P;
    int device = 0;
    std::string err;                    // last_error
    bool begun = false;                 // a header, bam_begin or feed call has been made
    bool finished = false, seen_header = false;
    bool broken = false;                // a container error ended the run
    int fmt = FMT_SAM;                  // the current file's format
    int32_t floor_score = ev::MINAS;
    double kernel_ms = 0;
    DevMem d_P, d_hist;                 // char, unsigned long long
    evt::Rows spill;
    Pipeline pipe;
    NameTable targets;                  // of the current file
    BamStream bam;
    Outcome out;
    BreakdownRun bd;
    TruthRun tr;
};

namespace {

#define CK(x)                                                                                         \
    do {                                                                                              \
        hipError_t e_ = (x);                                                                          \
        if (e_ != hipSuccess) {                                                                       \
            c->err = std::string("HIP error: ") + hipGetErrorString(e_) + " at " #x;                  \
            return DWGSIM_HIP_ERR_DEVICE;                                                             \
        }                                                                                             \
    } while (0)

// buffers for `cap` text bytes: a line has at least its newline (ends, flags: cap entries); a record that reaches the histogram has at least
// 11 bytes (ten tabs and the newline), so the spill list needs fewer than cap / 8 entries.  Each buffer of a smaller slot is freed before its
// successor is made; the text buffer comes last, so that its capacity -- the slot's -- is the new one only once all the others were made.
int slot_alloc(dwgsim_hip_eval_ctx *c, Slot &S, size_t cap)
{
    auto exact = [](auto &b, size_t n) { return b.reserve(n, n); };
    CK(exact(S.h_res, sizeof(EvalRes)));
    CK(exact(S.d_text, cap + 16));
    CK(exact(S.d_ends, cap * sizeof(uint32_t)));
    CK(exact(S.d_tiles, (cap / EVAL_TILE + 1) * sizeof(uint32_t)));
    CK(exact(S.d_res, sizeof(EvalRes)));
    CK(exact(S.d_spill, (cap / 8 + 1) * sizeof(uint64_t)));
    CK(exact(S.d_flags, cap));
    CK(exact(S.h_offs, (cap / ev::BAM_FIXED + 8) * sizeof(uint32_t)));       // a whole BAM record has more than 32 bytes
    CK(exact(S.h_text, cap));
    return DWGSIM_HIP_OK;
}

// a device copy of n host bytes, in a buffer of exactly n bytes (the one it replaces is freed first)
int upload(dwgsim_hip_eval_ctx *c, DevMem &b, const void *src, size_t n)
{
    b.reset();
    CK(b.reserve(n, n));
    CK(hipMemcpy(b.get(), src, n, hipMemcpyHostToDevice));
    return DWGSIM_HIP_OK;
}

std::string error_block(const char *fn, const char *var, const char *msg, bool fatal)
{
    std::string s = BREAK_LINE;
    s += std::string("\rIn function \"") + fn + "\": " + (fatal ? "Fatal Error" : "Warning") + "[OutOfRange]. ";
    if (var) s += std::string("Variable/Value: ") + var + ".\n";
    s += std::string("Message: ") + msg + ".\n";
    s += fatal ? " ***** Exiting due to errors *****\n" : " ***** Warning *****\n";
    s += BREAK_LINE;
    return s;
}

// the message of the fatal record `line`: the reference prints the read name as it stood when it gave up
std::string fatal_text(const dwgsim_hip_eval_ctx *c, int code, const std::string &line)
{
    std::string var;
    size_t qlen = line.find('\t');
    if (qlen == std::string::npos) qlen = line.size();
    if (code == ev::E_PREFIX || code == ev::E_NAME || code == ev::E_CONTIG) {
        const ev::NameMask mk = ev::name_mask(line.data(), (int)qlen);
        for (size_t i = 0; i < qlen; ++i) var += mk.has((int)i) ? ' ' : line[i];
        if (code != ev::E_PREFIX && c->o.P) {
            const size_t pl = c->P.size();
            var = qlen > pl ? var.substr(pl + 1) : std::string();
        }
    }
    switch (code) {
    case ev::E_MALFORMED: return error_block("process_bam", nullptr, "[dwgsim_eval-hip] malformed SAM record", true);      // (BAM too: the model's wording)
    case ev::E_PREFIX: return error_block("process_bam", var.c_str(), "[dwgsim_eval] could not match read name with given read name prefix (-P)", true);
    case ev::E_NAME: return error_block("process_bam", var.c_str(), "[dwgsim_eval] read was not generated by dwgsim?", true);
    case ev::E_CONTIG:
        return error_block("process_bam", var.c_str(), "[dwgsim_eval] the mapped contig does not exist in the SAM header; perhaps you have a read name prefix?", true);
    case ev::E_RANDOM_CORRECT:
        return error_block("dwgsim_eval_counts_add", "predicted_value", "predicted value cannot be mapped correctly when the read is unmappable", true);
    case ev::E_PAIRED: return error_block("run", nullptr, "Found a read that was paired end", true);
    default: return error_block("run", nullptr, "Found a read that was not paired", true);
    }
}

ev::Opts dev_opts(const dwgsim_hip_eval_ctx *c)
{
    ev::Opts o;
    o.a = c->o.a; o.d = c->o.d; o.g = c->o.g; o.q = c->o.q; o.e = c->o.e; o.s = c->o.s; o.i = c->o.i; o.z = c->o.z; o.m = c->o.m;
    o.P_len = c->o.P ? (int32_t)c->P.size() : -1;
    o.P = c->d_P.get<char>();
    return o;
}

EvalRecArgs rec_args(dwgsim_hip_eval_ctx *c, const uint8_t *text, uint32_t *ends, EvalRes *res, uint64_t *spill, uint8_t *flags, uint32_t has_ctx)
{
    EvalRecArgs A;
    A.text = text; A.ends = ends; A.res = res; A.hist = c->d_hist.get<unsigned long long>(); A.spill = spill; A.flags = flags; A.has_ctx = has_ctx;
    A.win_lo = WIN_LO; A.floor_score = c->floor_score; A.opt = dev_opts(c); A.tg = c->targets.tg;
    return A;
}

EvalBdArgs bd_args(dwgsim_hip_eval_ctx *c)
{
    const evt::Breakdown &b = c->bd.b;
    EvalBdArgs B;
    B.hist = c->bd.d_hist.get<unsigned long long>(); B.n_rows = (uint32_t)b.n_rows; B.win = b.win; B.win_lo = b.win_lo; B.cap = b.cap;
    B.row_snps = b.row[ev::D_SNPS]; B.row_errors = b.row[ev::D_ERRORS]; B.row_indels = b.row[ev::D_INDELS]; B.row_end = b.row[ev::D_END];
    return B;
}

EvalTruthArgs truth_args(dwgsim_hip_eval_ctx *c)
{
    EvalTruthArgs T;
    T.slots = c->tr.d_slots.get<unsigned long long>(); T.mask = c->tr.mask; T.recs = c->tr.d_recs.get<ev::TruthRec>(); T.pool = c->tr.d_pool.get<uint32_t>();
    T.tmap = c->tr.d_tmap.get<int32_t>(); T.ctrs = c->tr.d_ctrs.get<unsigned long long>();
    return T;
}

// the kernels of one chunk in the form that the run uses: `size` bytes of SAM lines, or `size` BAM records behind the context record
void launch(dwgsim_hip_eval_ctx *c, hipStream_t st, const EvalRecArgs &A, int fmt, uint64_t size, uint32_t *tiles)
{
    const EvalBdArgs B = bd_args(c);
    const EvalTruthArgs T = truth_args(c);
    const EvalBdArgs *bd = c->bd.b.on ? &B : nullptr;
    const EvalTruthArgs *tr = c->tr.committed ? &T : nullptr;
    if (fmt == FMT_BAM) launch_eval_bam_chunk(st, A, bd, tr, (uint32_t)size);
    else launch_eval_chunk(st, A, bd, tr, size, tiles);
}

// the results of the oldest submitted chunk
int process_oldest(dwgsim_hip_eval_ctx *c)
{
    const int k = c->pipe.pending.front();
    c->pipe.pending.pop_front();
    Slot &S = c->pipe.s[k];
    CK(hipStreamSynchronize(S.st.get()));
    S.busy = false;
    float ms = 0;
    if (hipEventElapsedTime(&ms, S.e0.get(), S.e1.get()) == hipSuccess) c->kernel_ms += ms;
    if (c->out.failed) return DWGSIM_HIP_OK;
    const EvalRes r = *S.h_res.get<EvalRes>();
    const uint32_t n_rec = r.n_lines - S.has_ctx;
    if (r.err != ~0ull) {
        const uint64_t rec = r.err >> 8;
        c->out.failed = true;
        c->out.code = (int)(r.err & 0xff);
        c->out.err_rec = c->out.records + rec;
        if (S.fmt == FMT_BAM) {
            c->out.err_line.clear();
            if (c->out.code != ev::E_MALFORMED) bam::record_to_sam(S.h_text.get() + S.h_offs.get<uint32_t>()[rec + S.has_ctx], c->bam.bh, c->out.err_line);
            return DWGSIM_HIP_OK;
        }
        const char *p = S.h_text.get<char>();
        for (uint64_t i = 0; i < rec + S.has_ctx; ++i) p = (const char *)memchr(p, '\n', S.h_text.get<char>() + S.len - p) + 1;
        c->out.err_line.assign(p, (const char *)memchr(p, '\n', S.h_text.get<char>() + S.len - p) - p);
        return DWGSIM_HIP_OK;
    }
    c->out.n += r.n;
    c->out.records += n_rec;
    if (r.n_spill) {
        std::vector<uint64_t> sp(r.n_spill);
        CK(hipMemcpy(sp.data(), S.d_spill.get<uint64_t>(), sp.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
        if (c->bd.b.on) for (uint64_t w : sp) c->bd.spill.add_spill(c->bd.b, w, &c->spill);
        else for (uint64_t w : sp) c->spill[(int32_t)(uint32_t)(w >> 32)][(int)(w & 7)]++;
    }
    if (c->o.p && n_rec) {
        std::vector<uint8_t> fl(n_rec);
        CK(hipMemcpy(fl.data(), S.d_flags.get(), n_rec, hipMemcpyDeviceToHost));
        if (S.fmt == FMT_BAM) {
            for (uint32_t i = 0; i < n_rec; ++i)
                if (fl[i]) {
                    bam::record_to_sam(S.h_text.get() + S.h_offs.get<uint32_t>()[i + S.has_ctx], c->bam.bh, c->out.incorrect);
                    c->out.incorrect += '\n';
                }
            return DWGSIM_HIP_OK;
        }
        const char *p = S.h_text.get<char>() + S.ctx_len, *end = S.h_text.get<char>() + S.len;
        for (uint32_t i = 0; i < n_rec; ++i) {
            const char *e = (const char *)memchr(p, '\n', end - p) + 1;
            if (fl[i]) c->out.incorrect.append(p, e - p);
            p = e;
        }
    }
    return DWGSIM_HIP_OK;
}

int drain(dwgsim_hip_eval_ctx *c)
{
    while (!c->pipe.pending.empty()) {
        const int r = process_oldest(c);
        if (r) return r;
    }
    return DWGSIM_HIP_OK;
}

// The filling slot's chunk [0, cut) is on its stream: the other slot becomes the filling one (its results are read first when it is still
// busy) and starts with the chunk's last record [lb, cut), the context record, and what follows the chunk.
int hand_over(dwgsim_hip_eval_ctx *c, size_t cut, size_t lb)
{
    Slot &S = c->pipe.filling();
    S.busy = true;
    c->pipe.pending.push_back(c->pipe.cur);
    c->pipe.cur ^= 1;
    Slot &T = c->pipe.filling();
    if (T.busy) {
        const int r = process_oldest(c);
        if (r) return r;
    }
    const size_t ctx = cut - lb, rest = S.fill - cut;
    memcpy(T.h_text.get<char>(), S.h_text.get<char>() + lb, ctx);
    memcpy(T.h_text.get<char>() + ctx, S.h_text.get<char>() + cut, rest);
    T.ctx_len = ctx; T.has_ctx = 1; T.fill = ctx + rest; T.fmt = S.fmt;
    S.fill = 0;
    return DWGSIM_HIP_OK;
}

// Submit the filling slot's chunk [0, cut) and continue in the other slot with the chunk's last record and what follows the chunk.
// SAM: `cut` is just past a newline.  BAM: `cut` is the slot's hop, the end of its last whole record; the offsets go up with the text, the
// device is told their number instead of counting newlines, and the new slot's offset list starts with its context record.
int submit(dwgsim_hip_eval_ctx *c, size_t cut)
{
    Slot &S = c->pipe.filling();
    const bool bam = S.fmt == FMT_BAM;
    const uint32_t n = bam ? S.n_offs : 0;
    hipStream_t st = S.st.get();
    EvalRes *hres = S.h_res.get<EvalRes>(), *dres = S.d_res.get<EvalRes>();
    S.len = cut;
    *hres = EvalRes{~0ull, 0, n, 0};
    CK(hipEventRecord(S.e0.get(), st));
    CK(hipMemcpyAsync(S.d_text.get(), S.h_text.get<char>(), cut, hipMemcpyHostToDevice, st));
    if (bam) CK(hipMemcpyAsync(S.d_ends.get(), S.h_offs.get(), n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    CK(hipMemcpyAsync(dres, hres, sizeof(EvalRes), hipMemcpyHostToDevice, st));
    const EvalRecArgs A = rec_args(c, S.d_text.get(), S.d_ends.get<uint32_t>(), dres, S.d_spill.get<uint64_t>(), c->o.p ? S.d_flags.get() : nullptr, S.has_ctx);
    launch(c, st, A, S.fmt, bam ? n - S.has_ctx : cut, S.d_tiles.get<uint32_t>());
    CK(hipGetLastError());
    CK(hipMemcpyAsync(hres, dres, sizeof(EvalRes), hipMemcpyDeviceToHost, st));
    CK(hipEventRecord(S.e1.get(), st));
    // where the chunk's last record starts
    size_t lb = bam ? S.h_offs.get<uint32_t>()[n - 1] : cut - 1;
    while (!bam && lb > 0 && S.h_text.get<char>()[lb - 1] != '\n') --lb;
    if (const int r = hand_over(c, cut, lb)) return r;
    if (bam) {
        Slot &T = c->pipe.filling();
        T.h_offs.get<uint32_t>()[0] = 0;
        T.n_offs = 1; T.hop = T.ctx_len;
        S.n_offs = 0; S.hop = 0;
    }
    return DWGSIM_HIP_OK;
}

// twice the room in both slots (a line longer than the filling slot's free space after its context line)
int grow(dwgsim_hip_eval_ctx *c)
{
    int r = drain(c);
    if (r) return r;
    Slot &F = c->pipe.filling();
    const size_t cap = F.h_text.cap() * 2;
    std::string keep(F.h_text.get<char>(), F.fill);
    for (Slot &S : c->pipe.s) if ((r = slot_alloc(c, S, cap))) return r;
    memcpy(F.h_text.get<char>(), keep.data(), keep.size());
    if (F.fmt == FMT_BAM && F.has_ctx) F.h_offs.get<uint32_t>()[0] = 0;      // (grow is for a slot without a whole record behind its context)
    return DWGSIM_HIP_OK;
}

int end_bam_file(dwgsim_hip_eval_ctx *c);

// the filling slot's complete lines, and a last line without its newline
int end_file(dwgsim_hip_eval_ctx *c)
{
    if (c->broken) return DWGSIM_HIP_ERR_FAILED;
    if (c->fmt == FMT_BAM) return end_bam_file(c);
    Slot &F = c->pipe.filling();
    if (F.fill > F.ctx_len && F.h_text.get<char>()[F.fill - 1] != '\n') {
        if (F.fill == F.h_text.cap()) {
            const int r = grow(c);
            if (r) return r;
        }
        Slot &G = c->pipe.filling();
        G.h_text.get<char>()[G.fill++] = '\n';
    }
    Slot &H = c->pipe.filling();
    if (H.fill > H.ctx_len && !c->out.failed) {
        const int r = submit(c, H.fill);
        if (r) return r;
    }
    return drain(c);
}

// the device copies of a name table, and its ev::Targets over them
int upload_names(dwgsim_hip_eval_ctx *c, NameTable &t)
{
    if (const int r = upload(c, t.d_names, t.names.data(), t.names.size() + 1)) return r;
    if (const int r = upload(c, t.d_off, t.off.data(), t.off.size() * sizeof(uint32_t))) return r;
    if (const int r = upload(c, t.d_hash, t.hash.data(), t.hash.size() * sizeof(int32_t))) return r;
    t.tg = {t.d_names.get<char>(), t.d_off.get<uint32_t>(), t.d_hash.get<int32_t>(), t.n(), (uint32_t)t.hash.size() - 1};
    return DWGSIM_HIP_OK;
}

// with a truth: for every target of the current file the truth contig of the same name, or -1
int map_contigs(dwgsim_hip_eval_ctx *c, const NameTable &file, const NameTable &truth)
{
    if (!c->tr.committed) return DWGSIM_HIP_OK;
    const ev::Targets T = truth.host();
    std::vector<int32_t> map(file.off.size(), -1);        // (one more than the targets: never empty)
    for (int32_t t = 0; t < file.n(); ++t) map[t] = ev::target_find(T, file.names.data() + file.off[t], file.off[t + 1] - file.off[t]);
    return upload(c, c->tr.d_tmap, map.data(), map.size() * sizeof(int32_t));
}

// c->targets (from the @SQ names of a SAM header, or the reference list of a BAM file) on the device, and mapped to the truth's contigs
int upload_targets(dwgsim_hip_eval_ctx *c)
{
    if (const int r = upload_names(c, c->targets)) return r;
    return map_contigs(c, c->targets, c->tr.contigs);
}

// ---- BAM stream ----

// The record at offset `at` of `fill` bytes of BAM records: its size, block_size field included, when all of it is there; 0 when it is not
// there yet; -1 when its block_size is one that no record can have.
int64_t whole_record(const uint8_t *t, size_t fill, size_t at)
{
    if (fill - at < 4) return 0;
    const uint32_t bs = bam::le32(t + at);
    if (bs < ev::BAM_FIXED || bs > ev::BAM_MAX_BLOCK) return -1;
    return fill - at - 4 < bs ? 0 : 4 + (int64_t)bs;
}

// the whole records that the filling slot's new bytes complete; a block_size that no record can have ends the stream with that record
void hop_records(dwgsim_hip_eval_ctx *c)
{
    Slot &F = c->pipe.filling();
    uint32_t *offs = F.h_offs.get<uint32_t>();
    int64_t k;
    for (; (k = whole_record(F.h_text.get(), F.fill, F.hop)) > 0; F.hop += (size_t)k) offs[F.n_offs++] = (uint32_t)F.hop;
    if (k < 0) {
        offs[F.n_offs++] = (uint32_t)F.hop;
        F.hop += 4;
        F.fill = F.hop;
        c->bam.bam_stop = true;
    }
}

// `need` free bytes in the filling slot: its whole records are submitted, or, when it has none, both slots grow
int bam_room(dwgsim_hip_eval_ctx *c, size_t need)
{
    for (;;) {
        Slot &F = c->pipe.filling();
        if (F.h_text.cap() - F.fill >= need) return DWGSIM_HIP_OK;
        const int r = F.n_offs > F.has_ctx ? submit(c, F.hop) : grow(c);
        if (r) return r;
    }
}

// A container error at byte `at` of the compressed file.  The whole records in front of it are evaluated first: a fatal record wins.
int container_error(dwgsim_hip_eval_ctx *c, const char *why, uint64_t at)
{
    Slot &F = c->pipe.filling();
    int r = DWGSIM_HIP_OK;
    if (F.n_offs > F.has_ctx && !c->out.failed) r = submit(c, F.hop);
    if (!r) r = drain(c);
    if (r) return r;
    if (c->out.failed) return DWGSIM_HIP_EVAL_STOPPED;
    char buf[64];
    snprintf(buf, sizeof buf, " at byte %llu of the compressed file", (unsigned long long)at);
    c->err = std::string("BAM input: ") + why + buf;
    c->broken = true;
    return DWGSIM_HIP_ERR_FAILED;
}

// the header is complete: targets, the -p header text, and the bytes behind it as the first record bytes
int bam_header_done(dwgsim_hip_eval_ctx *c, size_t hlen)
{
    c->bam.in_header = false;
    if (!c->seen_header && c->o.p) c->out.incorrect = c->bam.bh.text;
    c->seen_header = true;
    c->targets.from_names(c->bam.bh.names, c->bam.bh.off);
    int r = upload_targets(c);
    if (r) return r;
    const size_t rest = c->bam.hdr_bytes.size() - hlen;
    if ((r = bam_room(c, rest))) return r;
    Slot &F = c->pipe.filling();
    if (rest) memcpy(F.h_text.get() + F.fill, c->bam.hdr_bytes.data() + hlen, rest);
    F.fill += rest;
    std::vector<uint8_t>().swap(c->bam.hdr_bytes);
    hop_records(c);
    return DWGSIM_HIP_OK;
}

// everything that the collected compressed bytes allow
int bam_pump(dwgsim_hip_eval_ctx *c)
{
    if (!c->bam.pool) c->bam.pool.reset(new bam::InflatePool(c->bam.inflate_threads));
    while (!c->out.failed && !c->bam.bam_stop) {
        const uint8_t *z = c->bam.zbuf.data() + c->bam.zhead;
        const size_t avail = c->bam.zbuf.size() - c->bam.zhead;
        const char *why = nullptr;
        bam::BgzfBlock b;
        if (c->bam.in_header) {
            const int k = bam::bgzf_block_at(z, avail, &b, &why);
            if (k == 0) break;
            if (k < 0) return container_error(c, why, c->bam.zpos);
            const size_t at = c->bam.hdr_bytes.size();
            c->bam.hdr_bytes.resize(at + b.isize);
            bam::InflateJob j = {z + b.data_off, b.data_len, c->bam.hdr_bytes.data() + at, b.isize, b.crc, nullptr};
            bam::inflate_blocks(*c->bam.pool, &j, 1);
            if (j.error) return container_error(c, j.error, c->bam.zpos);
            c->bam.zhead += b.size; c->bam.zpos += b.size;
            const int64_t hl = bam::parse_header(c->bam.hdr_bytes.data(), c->bam.hdr_bytes.size(), &c->bam.bh, &why);
            if (hl < 0) return container_error(c, why, c->bam.zpos);
            if (hl > 0) {
                const int r = bam_header_done(c, (size_t)hl);
                if (r) return r;
            }
            continue;
        }
        // the complete blocks that fit into the filling slot, each at the place that the ISIZE values in front of it give
        Slot *F = &c->pipe.filling();
        size_t room = F->h_text.cap() - F->fill, used = 0, zused = 0;
        c->bam.jobs.clear();
        int k;
        while ((k = bam::bgzf_block_at(z + zused, avail - zused, &b, &why)) == 1 && c->bam.jobs.size() < MAX_BATCH) {
            if (b.isize > room - used) {
                if (!c->bam.jobs.empty()) break;
                const int r = bam_room(c, b.isize);
                if (r) return r;
                F = &c->pipe.filling();
                room = F->h_text.cap() - F->fill;
            }
            c->bam.jobs.push_back({z + zused + b.data_off, b.data_len, F->h_text.get() + F->fill + used, b.isize, b.crc, nullptr});
            used += b.isize; zused += b.size;
        }
        if (c->bam.jobs.empty() && k == 0) break;
        bam::inflate_blocks(*c->bam.pool, c->bam.jobs.data(), c->bam.jobs.size());
        // the blocks in front of the first bad one count
        size_t zgood = 0;
        const uint8_t *zb = z;
        for (const bam::InflateJob &j : c->bam.jobs) {
            if (j.error) { why = j.error; k = -1; break; }
            F->fill += j.isize;
            bam::bgzf_block_at(zb, avail - zgood, &b, &why);
            zgood += b.size; zb += b.size;
        }
        c->bam.zhead += zgood; c->bam.zpos += zgood;
        hop_records(c);
        if (c->bam.bam_stop) break;
        if (k < 0) return container_error(c, why, c->bam.zpos);
    }
    if (c->bam.bam_stop && !c->out.failed) {
        // the record that cannot be one is the last of the stream
        int r = submit(c, c->pipe.filling().hop);
        if (!r) r = drain(c);
        if (r) return r;
    }
    return c->out.failed ? DWGSIM_HIP_EVAL_STOPPED : DWGSIM_HIP_OK;
}

void bam_compact(dwgsim_hip_eval_ctx *c)
{
    c->bam.zbuf.erase(c->bam.zbuf.begin(), c->bam.zbuf.begin() + (ptrdiff_t)c->bam.zhead);
    c->bam.zhead = 0;
}

// the end of a BAM file: it must end at a block boundary, behind the header, and between two records
int end_bam_file(dwgsim_hip_eval_ctx *c)
{
    Slot &F = c->pipe.filling();
    if (!c->out.failed && !c->bam.bam_stop) {
        const char *why = c->bam.zbuf.size() > c->bam.zhead ? "the file ends inside a BGZF block" : c->bam.in_header ? "the file ends inside the BAM header"
                        : F.fill > F.hop ? "the file ends inside a record" : nullptr;
        if (why) {
            // (a fatal record in front of the end is the run's result, not an error of this call)
            const int r = container_error(c, why, c->bam.zpos + (c->bam.zbuf.size() - c->bam.zhead));
            return r == DWGSIM_HIP_EVAL_STOPPED ? DWGSIM_HIP_OK : r;
        }
    }
    if (F.n_offs > F.has_ctx && !c->out.failed) {
        const int r = submit(c, F.hop);
        if (r) return r;
    }
    c->bam.zbuf.clear(); c->bam.zhead = 0;
    return drain(c);
}

// The context record of the filling slot in the format of the file that begins (-m compares across files of different formats): a record
// of the other format with the same QNAME and FLAG.  A name that the other format cannot hold equals no name there: no context then.
void convert_ctx(dwgsim_hip_eval_ctx *c, int fmt)
{
    Slot &F = c->pipe.filling();
    if (F.has_ctx && F.fmt != fmt && !c->out.failed) {
        const ev::Prev pv = F.fmt == FMT_SAM ? ev::sam_prev(F.h_text.get<char>(), (uint32_t)F.ctx_len - 1) : ev::bam_prev(F.h_text.get());
        const std::string q(pv.qname, pv.qlen);
        std::string rec;
        const bool fits = !q.empty() && q.size() <= (size_t)ev::MAX_QNAME && q.find_first_of(fmt == FMT_SAM ? "\t\n" : std::string(1, '\0')) == std::string::npos;
        if (fits && fmt == FMT_SAM) {
            rec = q + "\t" + std::to_string(pv.flag) + "\n";
        } else if (fits) {
            rec.assign(4 + ev::BAM_FIXED, '\0');
            auto put32 = [&](size_t at, uint32_t v) { for (int k = 0; k < 4; ++k) rec[at + k] = (char)(v >> (8 * k)); };
            put32(0, ev::BAM_FIXED + (uint32_t)q.size() + 1);
            put32(4, ~0u); put32(8, ~0u); put32(24, ~0u); put32(28, ~0u);      // refID, pos, next_refID, next_pos: -1
            rec[12] = (char)(q.size() + 1);
            rec[18] = (char)(pv.flag & 0xff); rec[19] = (char)(pv.flag >> 8);
            rec += q;
            rec += '\0';
        }
        memcpy(F.h_text.get<char>(), rec.data(), rec.size());
        F.has_ctx = fits ? 1 : 0;
        F.ctx_len = F.fill = rec.size();
    }
    F.fmt = fmt;
    if (fmt == FMT_BAM) {
        if (F.has_ctx) F.h_offs.get<uint32_t>()[0] = 0;
        F.n_offs = F.has_ctx; F.hop = F.ctx_len;
    }
}

// ---- the truth (dw_eval.hpp TRUTH): load, index, text ----

int truth_fail(dwgsim_hip_eval_ctx *c, int rc, const std::string &msg)
{
    c->err = msg;
    c->tr.bad = true;
    return rc;
}

// room for `total` elements in a buffer that holds `have`: it doubles, and what it holds moves over
int truth_room(dwgsim_hip_eval_ctx *c, DevMem &buf, uint64_t have, uint64_t total, size_t elem, const char *what)
{
    if (total * elem <= buf.cap()) return DWGSIM_HIP_OK;
    DevMem nb;
    const uint64_t twice = std::max<uint64_t>(2 * have, 4096);
    // (while it copies, the old and the new buffer exist side by side: up to three times the bytes held)
    if (nb.reserve(1, std::max(total, twice) * elem) != hipSuccess) {
        (void)hipGetLastError();        // the doubled size did not fit: the exact one may
        if (nb.reserve(1, total * elem) != hipSuccess) {
            (void)hipGetLastError();
            nb.reset();
        }
    }
    if (!nb) {
        return truth_fail(c, DWGSIM_HIP_ERR_NOMEM, std::string("truth: the ") + what + " do not fit in device memory");
    }
    if (have) CK(hipMemcpy(nb.get(), buf.get(), have * elem, hipMemcpyDeviceToDevice));
    buf = std::move(nb);
    return DWGSIM_HIP_OK;
}

const char *truth_line_error(int code)
{
    switch (code) {
    case ev::T_E_FIELDS: return "has fewer than 11 fields";
    case ev::T_E_FORMAT: return "is not a truth record (QNAME, FLAG, POS or the end bits of FLAG)";
    case ev::T_E_POS: return "is mapped at POS 0";
    case ev::T_E_RNAME: return "has an RNAME that is not one of the truth's @SQ names";
    default: return "has a CIGAR that is no sequence of M, I and D runs with a query base";
    }
}

// the whole lines h_text[0, cut) of slot 0: newline kernels, then count, scan and write, each sized by what the step before it produced
int truth_chunk(dwgsim_hip_eval_ctx *c, size_t cut)
{
    Slot &S = c->pipe.s[0];
    auto &T = c->tr;
    hipStream_t st = S.st.get();
    EvalRes *hres = S.h_res.get<EvalRes>(), *dres = S.d_res.get<EvalRes>();
    *hres = EvalRes{~0ull, 0, 0, 0};
    CK(hipMemcpyAsync(S.d_text.get(), S.h_text.get(), cut, hipMemcpyHostToDevice, st));
    CK(hipMemcpyAsync(dres, hres, sizeof(EvalRes), hipMemcpyHostToDevice, st));
    launch_eval_newlines(st, S.d_text.get(), cut, S.d_tiles.get<uint32_t>(), dres, S.d_ends.get<uint32_t>());
    CK(hipGetLastError());
    CK(hipMemcpyAsync(hres, dres, sizeof(EvalRes), hipMemcpyDeviceToHost, st));
    CK(hipStreamSynchronize(st));
    const uint32_t n = hres->n_lines;
    if (!n) return DWGSIM_HIP_OK;
    if (T.n_recs + n > 0xFFFFFFFEull) return truth_fail(c, DWGSIM_HIP_ERR_ARG, "truth: more than 2^32 - 2 records");
    if (const int r = truth_room(c, T.d_recs, T.n_recs, T.n_recs + n, sizeof(ev::TruthRec), "records")) return r;
    if (T.d_cnt.reserve((size_t)n * sizeof(uint32_t), (size_t)n * sizeof(uint32_t)) != hipSuccess || T.d_err.reserve(8, 8) != hipSuccess) {
        (void)hipGetLastError();
        return truth_fail(c, DWGSIM_HIP_ERR_NOMEM, "truth: the records do not fit in device memory");
    }
    EvalTruthLoadArgs L;
    L.text = S.d_text.get(); L.ends = S.d_ends.get<uint32_t>(); L.n_lines = n; L.cnt = T.d_cnt.get<uint32_t>(); L.tg = T.contigs.tg;
    L.recs = T.d_recs.get<ev::TruthRec>() + T.n_recs; L.pool = nullptr; L.pool_base = (uint32_t)T.n_pool; L.err = T.d_err.get<unsigned long long>();
    CK(hipMemsetAsync(T.d_err.get(), 0xff, 8, st));
    launch_truth_load(st, L, dres);
    CK(hipGetLastError());
    CK(hipMemcpyAsync(hres, dres, sizeof(EvalRes), hipMemcpyDeviceToHost, st));
    CK(hipStreamSynchronize(st));
    unsigned long long bad = 0;
    CK(hipMemcpy(&bad, T.d_err.get(), 8, hipMemcpyDeviceToHost));
    if (bad != ~0ull) {
        char buf[64];
        snprintf(buf, sizeof buf, "truth: record line %llu ", (unsigned long long)(T.n_recs + (bad >> 8) + 1));
        return truth_fail(c, DWGSIM_HIP_ERR_FAILED, std::string(buf) + truth_line_error((int)(bad & 0xff)));
    }
    const uint32_t words = hres->n_lines;       // (k_eval_scan leaves its total there)
    if (T.n_pool + words > 0xFFFFFFFFull) return truth_fail(c, DWGSIM_HIP_ERR_ARG, "truth: more than 2^32 - 1 CIGAR operations outside single M runs");
    if (const int r = truth_room(c, T.d_pool, T.n_pool, T.n_pool + words, sizeof(uint32_t), "CIGAR operations")) return r;
    L.pool = T.d_pool.get<uint32_t>();
    launch_truth_write(st, L);
    CK(hipGetLastError());
    CK(hipStreamSynchronize(st));
    T.n_recs += n; T.n_pool += words;
    return DWGSIM_HIP_OK;
}

int truth_state(dwgsim_hip_eval_ctx *c)
{
    if (!c || c->finished || c->begun || c->tr.committed) return DWGSIM_HIP_ERR_STATE;
    if (c->tr.bad) return DWGSIM_HIP_ERR_FAILED;
    if (c->bd.b.on) {
        c->err = "a breakdown and a truth in one context are not supported";
        return DWGSIM_HIP_ERR_ARG;
    }
    return hipSetDevice(c->device) == hipSuccess ? DWGSIM_HIP_OK : DWGSIM_HIP_ERR_DEVICE;
}

// the truth section of the output from the 64-bit counters (dw_eval_launch.hpp)
std::string truth_text(const std::vector<unsigned long long> &k)
{
    std::string s;
    for (int st = 0; st < 2; ++st) {
        s += st ? "## truth indel\n" : "## truth all\n";
        s += "# mapq\tmissing\trandom\tunusable\tcompared\texact\tbases\tright\tclipped\tibases\tiright\n";
        unsigned long long cum[EVAL_TR_COLS] = {0};
        bool any = false;
        auto row = [&](int q) {
            s += std::to_string(q);
            for (unsigned long long v : cum) s += '\t' + std::to_string(v);
            s += '\n';
        };
        for (int q = 255; q >= 0; --q) {
            const unsigned long long *r = &k[(size_t)(st * 256 + q) * EVAL_TR_COLS];
            if (!(r[TC_MISSING] + r[TC_RANDOM] + r[TC_UNUSABLE] + r[TC_COMPARED])) continue;
            any = true;
            for (int j = 0; j < EVAL_TR_COLS; ++j) cum[j] += r[j];
            row(q);
        }
        if (!any) row(0);
    }
    return s;
}

// the main table of a plain run: the spill lists' counts and the window h
void format_table(dwgsim_hip_eval_ctx *c, const std::vector<unsigned long long> &h)
{
    evt::Rows rows = c->spill;
    evt::add_window(rows, h.data(), EVAL_WIN, WIN_LO, c->floor_score);
    c->out.table = evt::table_text(rows, c->o.a, c->o.d);
}

// the main table and the sections of a breakdown run
void format_breakdown(dwgsim_hip_eval_ctx *c, const std::vector<unsigned long long> &counters)
{
    evt::Rows rows = c->spill;
    evt::add_main_window(c->bd.b, counters.data(), c->floor_score, &rows);
    c->out.table = evt::table_text(rows, c->o.a, c->o.d);
    c->bd.text = evt::breakdown_text(c->bd.b, c->bd.spill, counters.data(), c->floor_score, c->o.a, c->o.d);
}

// A file of format `fmt` begins: the file before it ends (its last chunk is submitted and every result read), and the filling slot's context
// record takes the new format.  Refused after finish() and while a truth is begun but not committed.
int begin_file(dwgsim_hip_eval_ctx *c, int fmt)
{
    if (!c || c->finished) return DWGSIM_HIP_ERR_STATE;
    if (c->tr.begun && !c->tr.committed) {
        c->err = "the truth is not committed";
        return DWGSIM_HIP_ERR_STATE;
    }
    if (hipSetDevice(c->device) != hipSuccess) return DWGSIM_HIP_ERR_DEVICE;
    c->begun = true;
    if (const int r = end_file(c)) return r;
    c->fmt = fmt;
    convert_ctx(c, fmt);
    return DWGSIM_HIP_OK;
}

} // namespace

extern "C" {

void dwgsim_hip_eval_opts_default(dwgsim_hip_eval_opts_t *o)
{
    memset(o, 0, sizeof *o);
    o->size = sizeof *o;        // (inflate_threads 0: the default)
    o->d = 1; o->e = -1; o->g = 5; o->s = -1;
}

dwgsim_hip_eval_ctx_t *dwgsim_hip_eval_create(const dwgsim_hip_eval_opts_t *opts, int device, int *err)
{
    int dummy;
    if (!err) err = &dummy;
    // (a caller built against ABI version 1 passes the options without inflate_threads)
    const size_t v1_size = offsetof(dwgsim_hip_eval_opts_t, inflate_threads);
    if (!opts || (opts->size != sizeof(dwgsim_hip_eval_opts_t) && opts->size != v1_size) || opts->d == 0 ||
        (opts->chunk_bytes && (opts->chunk_bytes < MIN_CHUNK || opts->chunk_bytes > MAX_CHUNK)) ||
        (opts->size > v1_size && opts->inflate_threads < 0)) {
        *err = DWGSIM_HIP_ERR_ARG;
        return nullptr;
    }
    auto *c = new dwgsim_hip_eval_ctx;
    dwgsim_hip_eval_opts_default(&c->o);
    memcpy(&c->o, opts, opts->size);
    c->o.size = sizeof c->o;
    if (c->o.inflate_threads) c->bam.inflate_threads = c->o.inflate_threads > MAX_INFLATE_THREADS ? MAX_INFLATE_THREADS : c->o.inflate_threads;
    if (opts->P) c->P = opts->P;
    c->o.P = opts->P ? c->P.c_str() : nullptr;
    c->device = device;
    c->floor_score = ev::cdiv(ev::MINAS, opts->d);
    if (c->floor_score < ev::MINAS) c->floor_score = ev::MINAS;
    auto fail = [&](int e) { dwgsim_hip_eval_destroy(c); *err = e; return (dwgsim_hip_eval_ctx_t *)nullptr; };
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || device < 0 || device >= nd || hipSetDevice(device) != hipSuccess) return fail(DWGSIM_HIP_ERR_DEVICE);
    const size_t cap = opts->chunk_bytes ? opts->chunk_bytes : DEFAULT_CHUNK;
    for (Slot &S : c->pipe.s) {
        if (slot_alloc(c, S, cap)) return fail(DWGSIM_HIP_ERR_DEVICE);
        if (S.st.create() != hipSuccess || S.e0.create() != hipSuccess || S.e1.create() != hipSuccess) return fail(DWGSIM_HIP_ERR_DEVICE);
    }
    const size_t hb = 5 * (EVAL_WIN + 1) * sizeof(unsigned long long);
    if (c->d_hist.reserve(hb, hb) != hipSuccess || hipMemset(c->d_hist.get(), 0, hb) != hipSuccess) return fail(DWGSIM_HIP_ERR_DEVICE);
    if (upload(c, c->d_P, c->P.c_str(), c->P.size() + 1)) return fail(DWGSIM_HIP_ERR_DEVICE);
    c->targets.from_sq("", 0);      // (no targets yet)
    if (upload_targets(c)) return fail(DWGSIM_HIP_ERR_DEVICE);
    *err = DWGSIM_HIP_OK;
    return c;
}

int dwgsim_hip_eval_header(dwgsim_hip_eval_ctx_t *c, const char *text, size_t len)
{
    if (const int r = begin_file(c, FMT_SAM)) return r;
    if (!c->seen_header && c->o.p) c->out.incorrect.assign(text, len);
    c->seen_header = true;
    c->targets.from_sq(text, len);
    return upload_targets(c);
}

int dwgsim_hip_eval_bam_begin(dwgsim_hip_eval_ctx_t *c)
{
    if (const int r = begin_file(c, FMT_BAM)) return r;
    c->bam.restart();
    return DWGSIM_HIP_OK;
}

int dwgsim_hip_eval_feed_bam(dwgsim_hip_eval_ctx_t *c, const void *buf, size_t len)
{
    if (!c || c->finished || c->fmt != FMT_BAM || (len && !buf)) return DWGSIM_HIP_ERR_STATE;
    if (c->broken) return DWGSIM_HIP_ERR_FAILED;
    if (hipSetDevice(c->device) != hipSuccess) return DWGSIM_HIP_ERR_DEVICE;
    if (c->out.failed || c->bam.bam_stop) return c->out.failed ? DWGSIM_HIP_EVAL_STOPPED : DWGSIM_HIP_OK;
    c->bam.zbuf.insert(c->bam.zbuf.end(), (const uint8_t *)buf, (const uint8_t *)buf + len);
    const int r = bam_pump(c);
    bam_compact(c);
    return r;
}

int dwgsim_hip_eval_feed(dwgsim_hip_eval_ctx_t *c, const char *buf, size_t len)
{
    if (!c || c->finished || c->fmt != FMT_SAM || (c->tr.begun && !c->tr.committed)) return DWGSIM_HIP_ERR_STATE;
    if (c->broken) return DWGSIM_HIP_ERR_FAILED;
    if (hipSetDevice(c->device) != hipSuccess) return DWGSIM_HIP_ERR_DEVICE;
    c->seen_header = c->begun = true;      // the first file's header is empty when feed comes first
    while (len && !c->out.failed) {
        Slot &F = c->pipe.filling();
        if (F.fill == F.h_text.cap()) {
            size_t cut = F.fill;
            while (cut > F.ctx_len && F.h_text.get<char>()[cut - 1] != '\n') --cut;
            const int r = cut > F.ctx_len ? submit(c, cut) : grow(c);
            if (r) return r;
            continue;
        }
        const size_t k = len < F.h_text.cap() - F.fill ? len : F.h_text.cap() - F.fill;
        memcpy(F.h_text.get<char>() + F.fill, buf, k);
        F.fill += k; buf += k; len -= k;
    }
    return c->out.failed ? DWGSIM_HIP_EVAL_STOPPED : DWGSIM_HIP_OK;
}

int dwgsim_hip_eval_finish(dwgsim_hip_eval_ctx_t *c, dwgsim_hip_eval_summary_t *sm)
{
    if (!c || c->finished || !sm || sm->size != sizeof(dwgsim_hip_eval_summary_t)) return c && c->finished ? DWGSIM_HIP_ERR_STATE : DWGSIM_HIP_ERR_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return DWGSIM_HIP_ERR_DEVICE;
    int r = end_file(c);
    if (r) return r;
    c->finished = true;
    c->out.stderr_text = "Analyzing...\nCurrently on:\n0";
    if (c->out.failed) {
        c->out.stderr_text += fatal_text(c, c->out.code, c->out.err_line);
        c->out.table.clear();
        c->out.incorrect.clear();
    } else {
        if (c->bd.b.on) {
            std::vector<unsigned long long> counters(c->bd.b.counters());
            CK(hipMemcpy(counters.data(), c->bd.d_hist.get(), counters.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
            format_breakdown(c, counters);
        } else {
            std::vector<unsigned long long> h(5 * (EVAL_WIN + 1));
            CK(hipMemcpy(h.data(), c->d_hist.get(), h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
            format_table(c, h);
        }
        if (c->tr.committed) {
            std::vector<unsigned long long> k(EVAL_TR_CTRS);
            CK(hipMemcpy(k.data(), c->tr.d_ctrs.get(), k.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
            c->tr.text = truth_text(k);
        }
        char buf[128];
        snprintf(buf, sizeof buf, "\r%llu\n", (unsigned long long)c->out.n);
        c->out.stderr_text += buf;
        if (c->o.n > 0 && c->out.n != (uint64_t)c->o.n) {
            snprintf(buf, sizeof buf, "(-n)=%d\tn=%llu\n", c->o.n, (unsigned long long)c->out.n);
            c->out.stderr_text += buf;
            c->out.stderr_text += error_block("run", nullptr, "Number of reads found differs from the number specified (-n)", false);
        }
        c->out.stderr_text += "Analysis complete.\n";
    }
    const uint32_t size = sm->size;
    memset(sm, 0, sizeof *sm);
    sm->size = size;
    sm->status = c->out.failed ? 1 : 0;
    sm->error_code = c->out.failed ? c->out.code : 0;
    sm->error_record = c->out.failed ? c->out.err_rec : 0;
    sm->n = c->out.n;
    sm->records = c->out.records;
    sm->stderr_text = c->out.stderr_text.c_str();
    sm->stderr_len = c->out.stderr_text.size();
    return DWGSIM_HIP_OK;
}

int dwgsim_hip_eval_table_text(dwgsim_hip_eval_ctx_t *c, const char **txt, size_t *len)
{
    if (!c || !c->finished || !txt || !len) return DWGSIM_HIP_ERR_STATE;
    *txt = c->out.table.c_str(); *len = c->out.table.size();
    return DWGSIM_HIP_OK;
}

int dwgsim_hip_eval_incorrect_text(dwgsim_hip_eval_ctx_t *c, const char **txt, size_t *len)
{
    if (!c || !c->finished || !txt || !len) return DWGSIM_HIP_ERR_STATE;
    *txt = c->out.incorrect.c_str(); *len = c->out.incorrect.size();
    return DWGSIM_HIP_OK;
}

int dwgsim_hip_eval_set_breakdown(dwgsim_hip_eval_ctx_t *c, const char *dims, int cap)
{
    if (!c || c->finished || c->begun) return DWGSIM_HIP_ERR_STATE;
    if (c->tr.begun && dims && *dims) {
        c->err = "a breakdown and a truth in one context are not supported";
        return DWGSIM_HIP_ERR_ARG;
    }
    evt::Breakdown b;
    if (const char *why = evt::parse_breakdown(dims, cap, c->o.a, EVAL_BD_CTRS, EVAL_WIN, &b)) {
        c->err = why;
        return DWGSIM_HIP_ERR_ARG;
    }
    if (hipSetDevice(c->device) != hipSuccess) return DWGSIM_HIP_ERR_DEVICE;
    c->bd.b = evt::Breakdown();
    c->bd.d_hist.reset();
    if (b.on) {
        const size_t bytes = b.counters() * sizeof(unsigned long long);
        CK(c->bd.d_hist.reserve(bytes, bytes));
        CK(hipMemset(c->bd.d_hist.get(), 0, bytes));
    }
    c->bd.b = b;
    return DWGSIM_HIP_OK;
}

int dwgsim_hip_eval_breakdown_text(dwgsim_hip_eval_ctx_t *c, const char **txt, size_t *len)
{
    if (!c || !c->finished || !txt || !len) return DWGSIM_HIP_ERR_STATE;
    *txt = c->bd.text.c_str(); *len = c->bd.text.size();
    return DWGSIM_HIP_OK;
}

int dwgsim_hip_eval_truth_header(dwgsim_hip_eval_ctx_t *c, const char *text, size_t len)
{
    if (const int r = truth_state(c)) return r;
    if (len && !text) return DWGSIM_HIP_ERR_ARG;
    auto &T = c->tr;
    if (T.fed) return DWGSIM_HIP_ERR_STATE;       // (the records already loaded hold contig indices of the header before)
    T.begun = true;
    T.contigs.from_sq(text, len);
    return upload_names(c, T.contigs);
}

int dwgsim_hip_eval_truth_feed(dwgsim_hip_eval_ctx_t *c, const char *buf, size_t len)
{
    if (const int r = truth_state(c)) return r;
    if (len && !buf) return DWGSIM_HIP_ERR_ARG;
    if (!c->tr.begun)
        if (const int r = dwgsim_hip_eval_truth_header(c, "", 0)) return r;      // (no header: no contigs, so only unmapped lines can pass)
    c->tr.fed = true;
    while (len) {
        Slot &F = c->pipe.s[0];
        char *t = F.h_text.get<char>();
        if (F.fill == F.h_text.cap()) {
            size_t cut = F.fill;
            while (cut > 0 && t[cut - 1] != '\n') --cut;
            if (!cut) {
                if (const int r = grow(c)) return r;
                continue;
            }
            if (const int r = truth_chunk(c, cut)) return r;
            memmove(t, t + cut, F.fill - cut);
            F.fill -= cut;
            continue;
        }
        const size_t k = len < F.h_text.cap() - F.fill ? len : F.h_text.cap() - F.fill;
        memcpy(t + F.fill, buf, k);
        F.fill += k; buf += k; len -= k;
    }
    return DWGSIM_HIP_OK;
}

int dwgsim_hip_eval_truth_commit(dwgsim_hip_eval_ctx_t *c)
{
    if (const int r = truth_state(c)) return r;
    if (!c->tr.begun)
        if (const int r = dwgsim_hip_eval_truth_header(c, "", 0)) return r;
    auto &T = c->tr;
    // what is left, and a last line without its newline
    if (c->pipe.s[0].fill) {
        if (c->pipe.s[0].h_text.get<char>()[c->pipe.s[0].fill - 1] != '\n') {
            if (c->pipe.s[0].fill == c->pipe.s[0].h_text.cap())
                if (const int r = grow(c)) return r;
            c->pipe.s[0].h_text.get<char>()[c->pipe.s[0].fill++] = '\n';
        }
        if (const int r = truth_chunk(c, c->pipe.s[0].fill)) return r;
        c->pipe.s[0].fill = 0;
    }
    // at least twice as many slots as records, a power of two (the test hook may force another size, which must leave one slot empty).  A slot's
    // number has 32 bits: beyond 2^31 records the factor of two gives way, and the table has 2^32 slots for at most 2^32 - 2 records
    int lg = 1;
    while (lg < 32 && (1ull << lg) < 2 * T.n_recs) ++lg;
    if (T.force_log2 >= 0) lg = T.force_log2;
    const uint64_t slots = 1ull << lg;
    if (slots <= T.n_recs) return truth_fail(c, DWGSIM_HIP_ERR_ARG, "truth: the forced table has no room for the records and an empty slot");
    if (T.d_slots.reserve(slots * 8, slots * 8) != hipSuccess || T.d_err.reserve(8, 8) != hipSuccess ||
        T.d_ctrs.reserve(EVAL_TR_CTRS * 8, EVAL_TR_CTRS * 8) != hipSuccess) {
        (void)hipGetLastError();
        return truth_fail(c, DWGSIM_HIP_ERR_NOMEM, "truth: the index does not fit in device memory");
    }
    T.mask = (uint32_t)(slots - 1);
    hipStream_t st = c->pipe.s[0].st.get();
    CK(hipMemsetAsync(T.d_slots.get(), 0xff, slots * 8, st));
    CK(hipMemsetAsync(T.d_err.get(), 0xff, 8, st));
    CK(hipMemsetAsync(T.d_ctrs.get(), 0, EVAL_TR_CTRS * 8, st));
    if (T.n_recs) launch_truth_index(st, T.d_slots.get<unsigned long long>(), T.mask, T.d_recs.get<ev::TruthRec>(), (uint32_t)T.n_recs, T.d_err.get<unsigned long long>());
    CK(hipGetLastError());
    CK(hipStreamSynchronize(st));
    unsigned long long bad = 0;
    CK(hipMemcpy(&bad, T.d_err.get(), 8, hipMemcpyDeviceToHost));
    if (bad != ~0ull) {
        char buf[160];
        snprintf(buf, sizeof buf, "truth: the truth holds read of record line %llu twice (its name and end are those of record line %llu)",
                 (unsigned long long)(bad >> 32) + 1, (unsigned long long)(uint32_t)bad + 1);
        return truth_fail(c, DWGSIM_HIP_ERR_FAILED, buf);
    }
    T.d_cnt.reset(); T.d_err.reset();
    T.contigs.drop_device();
    T.committed = true;
    return map_contigs(c, c->targets, T.contigs);
}

int dwgsim_hip_eval_truth_text(dwgsim_hip_eval_ctx_t *c, const char **txt, size_t *len)
{
    if (!c || !c->finished || !txt || !len) return DWGSIM_HIP_ERR_STATE;
    *txt = c->tr.text.c_str(); *len = c->tr.text.size();
    return DWGSIM_HIP_OK;
}

int dwgsim_hip_eval_debug_truth_slots(dwgsim_hip_eval_ctx_t *c, int log2_slots)
{
    if (!c || c->finished || c->begun || c->tr.committed) return DWGSIM_HIP_ERR_STATE;
    if (log2_slots < 1 || log2_slots > 32) return DWGSIM_HIP_ERR_ARG;
    c->tr.force_log2 = log2_slots;
    return DWGSIM_HIP_OK;
}

const char *dwgsim_hip_eval_last_error(const dwgsim_hip_eval_ctx_t *c) { return c ? c->err.c_str() : "no context"; }

void dwgsim_hip_eval_destroy(dwgsim_hip_eval_ctx_t *c)
{
    if (!c) return;
    hipSetDevice(c->device);
    for (Slot &S : c->pipe.s) if (S.st) hipStreamSynchronize(S.st.get());      // (by name: the members' destructors only give handles and memory back)
    delete c;
}

int dwgsim_hip_eval_debug_time(dwgsim_hip_eval_ctx_t *c, double *kernel_ms)
{
    if (!c || !kernel_ms) return DWGSIM_HIP_ERR_ARG;
    *kernel_ms = c->kernel_ms;
    return DWGSIM_HIP_OK;
}

int dwgsim_hip_eval_debug_device_chunk(dwgsim_hip_eval_ctx_t *c, const void *text, size_t len, int reps, double *ms)
{
    if (!c || !text || !len || len > MAX_CHUNK * 4ull || reps < 1 || !ms) return DWGSIM_HIP_ERR_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return DWGSIM_HIP_ERR_DEVICE;
    DevMem dev, ends, tiles, res, spill;
    DevEvent e0, e1;
    auto exact = [](DevMem &b, size_t n) { return b.reserve(n, n) != hipSuccess; };
    if (exact(dev, len + 16) || exact(ends, len * sizeof(uint32_t)) || exact(tiles, (len / EVAL_TILE + 1) * sizeof(uint32_t)) || exact(res, sizeof(EvalRes)) ||
        exact(spill, (len / 8 + 1) * sizeof(uint64_t)) || e0.create() || e1.create()) {
        c->err = "debug_device_chunk: out of device memory";
        return DWGSIM_HIP_ERR_NOMEM;
    }
    hipStream_t st = c->pipe.s[0].st.get();
    if (hipMemcpy(dev.get(), text, len, hipMemcpyHostToDevice) != hipSuccess) {
        c->err = "debug_device_chunk: upload failed";
        return DWGSIM_HIP_ERR_DEVICE;
    }
    int rc = DWGSIM_HIP_OK;
    const EvalRecArgs A = rec_args(c, dev.get(), ends.get<uint32_t>(), res.get<EvalRes>(), spill.get<uint64_t>(), nullptr, 0);
    hipEventRecord(e0.get(), st);
    for (int i = 0; i < reps; ++i) {
        hipMemsetAsync(res.get(), 0xff, 8, st);
        hipMemsetAsync(res.get() + 8, 0, sizeof(EvalRes) - 8, st);
        launch(c, st, A, FMT_SAM, len, tiles.get<uint32_t>());
    }
    hipEventRecord(e1.get(), st);
    if (hipStreamSynchronize(st) != hipSuccess) { c->err = "debug_device_chunk: kernel failed"; rc = DWGSIM_HIP_ERR_DEVICE; }
    float t = 0;
    hipEventElapsedTime(&t, e0.get(), e1.get());
    *ms = t / reps;
    return rc;
}

int dwgsim_hip_eval_debug_device_bam_chunk(dwgsim_hip_eval_ctx_t *c, const void *records, size_t len, int reps, double *ms)
{
    if (!c || !records || !len || len > MAX_CHUNK * 2ull || reps < 1 || !ms) return DWGSIM_HIP_ERR_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return DWGSIM_HIP_ERR_DEVICE;
    // the offsets of the whole records, as hop_records finds them
    std::vector<uint32_t> offs;
    int64_t k;
    for (size_t q = 0; (k = whole_record((const uint8_t *)records, len, q)) > 0; q += (size_t)k) offs.push_back((uint32_t)q);
    if (offs.empty()) return DWGSIM_HIP_ERR_ARG;
    const size_t n = offs.size();
    DevMem dev, d_offs, res, spill;
    DevEvent e0, e1;
    auto exact = [](DevMem &b, size_t k) { return b.reserve(k, k) != hipSuccess; };
    if (exact(dev, len) || exact(d_offs, n * sizeof(uint32_t)) || exact(res, sizeof(EvalRes)) || exact(spill, (n + 1) * sizeof(uint64_t)) || e0.create() || e1.create()) {
        c->err = "debug_device_bam_chunk: out of device memory";
        return DWGSIM_HIP_ERR_NOMEM;
    }
    hipStream_t st = c->pipe.s[0].st.get();
    const EvalRes init = {~0ull, 0, (uint32_t)n, 0};
    if (hipMemcpy(dev.get(), records, len, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_offs.get(), offs.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess) {
        c->err = "debug_device_bam_chunk: upload failed";
        return DWGSIM_HIP_ERR_DEVICE;
    }
    int rc = DWGSIM_HIP_OK;
    const EvalRecArgs A = rec_args(c, dev.get(), d_offs.get<uint32_t>(), res.get<EvalRes>(), spill.get<uint64_t>(), nullptr, 0);
    double total = 0;
    for (int i = 0; i < reps && rc == DWGSIM_HIP_OK; ++i) {
        // (the result words are set outside the timed span: a BAM chunk's count comes from the host)
        if (hipMemcpy(res.get(), &init, sizeof init, hipMemcpyHostToDevice) != hipSuccess) { rc = DWGSIM_HIP_ERR_DEVICE; break; }
        hipEventRecord(e0.get(), st);
        launch(c, st, A, FMT_BAM, n, nullptr);
        hipEventRecord(e1.get(), st);
        if (hipStreamSynchronize(st) != hipSuccess) { c->err = "debug_device_bam_chunk: kernel failed"; rc = DWGSIM_HIP_ERR_DEVICE; break; }
        float ms1 = 0;
        hipEventElapsedTime(&ms1, e0.get(), e1.get());
        total += ms1;
    }
    *ms = total / reps;
    return rc;
}

int dwgsim_hip_eval_debug_inflate(const void *bam_bytes, size_t len, int threads, int reps, double *ms, uint64_t *out_bytes)
{
    if (!bam_bytes || !len || threads < 1 || threads > MAX_INFLATE_THREADS || reps < 1 || !ms || !out_bytes) return DWGSIM_HIP_ERR_ARG;
    const uint8_t *z = (const uint8_t *)bam_bytes;
    std::vector<bam::InflateJob> jobs;
    uint64_t total = 0;
    for (size_t at = 0; at < len;) {
        bam::BgzfBlock b;
        const char *why;
        if (bam::bgzf_block_at(z + at, len - at, &b, &why) != 1) return DWGSIM_HIP_ERR_ARG;
        jobs.push_back({z + at + b.data_off, b.data_len, nullptr, b.isize, b.crc, nullptr});
        total += b.isize; at += b.size;
    }
    std::vector<uint8_t> out(total + 1);
    uint64_t to = 0;
    for (bam::InflateJob &j : jobs) { j.dst = out.data() + to; to += j.isize; }
    bam::InflatePool pool(threads);
    double best = 0;
    for (int i = 0; i < reps; ++i) {
        timespec t0, t1;
        clock_gettime(CLOCK_MONOTONIC, &t0);
        // in batches, as feed_bam hands them over
        for (size_t k = 0; k < jobs.size(); k += MAX_BATCH) bam::inflate_blocks(pool, jobs.data() + k, jobs.size() - k < MAX_BATCH ? jobs.size() - k : MAX_BATCH);
        clock_gettime(CLOCK_MONOTONIC, &t1);
        const double d = (t1.tv_sec - t0.tv_sec) * 1e3 + (t1.tv_nsec - t0.tv_nsec) * 1e-6;
        if (i == 0 || d < best) best = d;
        for (const bam::InflateJob &j : jobs) if (j.error) return DWGSIM_HIP_ERR_FAILED;
    }
    *ms = best;
    *out_bytes = total;
    return DWGSIM_HIP_OK;
}

} // extern "C"
