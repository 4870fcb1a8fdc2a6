// dw_eval.hip -- the kernels of dwgsim_eval-hip: SAM text in, per-score class counts out (host side: dw_eval.cpp; semantics: dw_eval.hpp).
//
// A chunk is whole lines of SAM record text (every line ends in '\n'), optionally led by one context line: the last record of the previous chunk,
// there only so that -m can compare the first record with the one before it.  Per chunk:
//   k_eval_count    newlines per 4 KiB tile
//   k_eval_scan     exclusive scan of the tile counts (one block), and the number of lines
//   k_eval_lines    the position of every newline, in order: line r = (ends[r-1], ends[r]]
//   k_eval_records  one lane per record: eval_records_loop behind the SAM front, in the run's form
// A chunk of a BAM file is whole binary records instead, led by the same kind of context record, and comes with the offset of every record:
//   k_eval_bam_records  the same loop behind the BAM front (parse_bam_record instead of parse_sam_line); the newline kernels are not launched.
//
// eval_records_loop is the per-record part, written once: parse, -m / -q / filters / class, the first fatal error (atomicMin of
// record << 8 | code), n, the -p flag.  Where a record that has a class is counted is its form's business; a run has one form:
//   Plain      (k_eval_records, k_eval_bam_records)  the histogram: an LDS window of EVAL_WIN scores x 5 classes plus one bin for the floor score
//              (the unmapped records of -a 1..3), merged into the 64-bit global histogram once per block; a score outside both goes to the spill
//              list, which the host adds.  The per-record (class, score) words never go to memory.
//   Breakdown  (k_eval_records_bd, k_eval_bam_records_bd; dw_eval.hpp BREAKDOWN)  once per selected dimension, in the record's stratum of that
//              dimension (EvalBdArgs lays the counters out).  A block has 512 lanes and 32 768 16-bit counters, two to an LDS word (64 KiB, two
//              blocks per CU); it merges them into the 64-bit global counters before any of them can reach 2^16, that is every BD_FLUSH_ITERS
//              turns of the record loop, and at its end.
//   Truth      (k_eval_records_tr, k_eval_bam_records_tr; dw_eval.hpp TRUTH)  Plain's count plus the join with the truth and the walk of the two
//              CIGARs, with 2 x 256 x 10 32-bit counters in LDS that are merged into 64-bit global ones every TR_FLUSH_ITERS turns.
// The truth SAM's own text goes through the same newline kernels; k_truth_count, k_eval_scan and k_truth_write turn every line into a 32-byte
// record and its CIGAR words, and k_truth_insert / k_truth_check build and verify the index at commit.
// The launchers at the end choose the kernel of a chunk from its front and the run's form, and its grid from that kernel's block size.
#include <hip/hip_runtime.h>
#include "dw_eval.hpp"
#include "dw_eval_launch.hpp"

namespace dw {

constexpr int EV_THREADS = 256;
constexpr int EV_BYTES = 16;                                 // per lane in the newline kernels
constexpr uint32_t EV_TILE = EV_THREADS * EV_BYTES;          // 4096

static_assert(EVAL_TILE == EV_TILE, "tile size");

// number of '\n' bytes in a 32-bit word (exact: no carries between bytes)
__device__ __forceinline__ uint32_t nl_count(uint32_t x)
{
    const uint32_t y = x ^ 0x0a0a0a0au;
    const uint32_t t = ~(((y & 0x7f7f7f7fu) + 0x7f7f7f7fu) | y | 0x7f7f7f7fu);
    return (uint32_t)__popc(t);
}

// the 16 bytes of a lane, as four words (past the end: zero bytes, which are no newline)
__device__ __forceinline__ void load16(const uint8_t *text, uint64_t len, uint64_t at, uint32_t w[4])
{
    if (at + EV_BYTES <= len) {
        const uint4 v = *(const uint4 *)(text + at);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    } else {
        for (int k = 0; k < 4; ++k) {
            uint32_t x = 0;
            for (int b = 0; b < 4; ++b) {
                const uint64_t p = at + 4 * k + b;
                x |= (uint32_t)(p < len ? text[p] : 0) << (8 * b);
            }
            w[k] = x;
        }
    }
}

// exclusive scan of one value per lane over the block (256 lanes), and the block total
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t *total)
{
    __shared__ uint32_t s[EV_THREADS];
    const int t = threadIdx.x;
    s[t] = v;
    __syncthreads();
    for (int d = 1; d < EV_THREADS; d <<= 1) {
        const uint32_t x = t >= d ? s[t - d] : 0;
        __syncthreads();
        s[t] += x;
        __syncthreads();
    }
    const uint32_t incl = s[t];
    *total = s[EV_THREADS - 1];
    __syncthreads();
    return incl - v;
}

__global__ __launch_bounds__(EV_THREADS) void k_eval_count(const uint8_t *text, uint64_t len, uint32_t *tile_count)
{
    uint32_t w[4];
    load16(text, len, (uint64_t)blockIdx.x * EV_TILE + threadIdx.x * EV_BYTES, w);
    const uint32_t c = nl_count(w[0]) + nl_count(w[1]) + nl_count(w[2]) + nl_count(w[3]);
    uint32_t tot;
    block_excl_scan(c, &tot);
    if (threadIdx.x == 0) tile_count[blockIdx.x] = tot;
}

__global__ __launch_bounds__(EV_THREADS) void k_eval_scan(uint32_t *tile_count, uint32_t n_tiles, EvalRes *res)
{
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n_tiles; base += EV_THREADS) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < n_tiles ? tile_count[i] : 0;
        uint32_t tot;
        const uint32_t ex = block_excl_scan(v, &tot);
        if (i < n_tiles) tile_count[i] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) res->n_lines = carry;
}

__global__ __launch_bounds__(EV_THREADS) void k_eval_lines(const uint8_t *text, uint64_t len, const uint32_t *tile_base, uint32_t *ends)
{
    const uint64_t at = (uint64_t)blockIdx.x * EV_TILE + threadIdx.x * EV_BYTES;
    uint32_t w[4];
    load16(text, len, at, w);
    const uint32_t c = nl_count(w[0]) + nl_count(w[1]) + nl_count(w[2]) + nl_count(w[3]);
    uint32_t tot;
    uint32_t o = tile_base[blockIdx.x] + block_excl_scan(c, &tot);
    if (!c) return;
    for (int k = 0; k < 4; ++k)
        for (int b = 0; b < 4; ++b)
            if (((w[k] >> (8 * b)) & 0xff) == '\n') ends[o++] = (uint32_t)(at + 4 * k + b);
}

// The two record fronts.  Record li of the chunk (the context record, when there is one, is record 0) becomes an ev::Rec, and the record in
// front of it an ev::Prev; everything after that is the same for both formats (eval_records_loop).
struct SamFront {
    // line li = (ends[li-1], ends[li])
    static __device__ __forceinline__ bool rec(const EvalRecArgs &A, uint32_t li, ev::Rec *r)
    {
        const uint32_t b = li ? A.ends[li - 1] + 1 : 0, e = A.ends[li];
        return ev::parse_sam_line((const char *)A.text + b, e - b, r);
    }
    static __device__ __forceinline__ ev::Prev prev(const EvalRecArgs &A, uint32_t li)
    {
        const uint32_t pb = li >= 2 ? A.ends[li - 2] + 1 : 0, pe = A.ends[li - 1];
        return ev::sam_prev((const char *)A.text + pb, pe - pb);
    }
};

struct BamFront {
    // record li starts at ends[li] (its block_size field); the host has checked that all of it lies inside the chunk
    static __device__ __forceinline__ bool rec(const EvalRecArgs &A, uint32_t li, ev::Rec *r)
    {
        const uint8_t *p = A.text + A.ends[li];
        return ev::parse_bam_record(p, ev::ld32(p), A.tg.n, r);
    }
    static __device__ __forceinline__ ev::Prev prev(const EvalRecArgs &A, uint32_t li) { return ev::bam_prev(A.text + A.ends[li - 1]); }
};

// ---- the three forms ----
// A form says where a record that has a class is counted, and nothing else.  It has the lanes of its blocks (THREADS), its LDS counters
// (zero(); merge(): the block's nonzero counters into the 64-bit global ones, and zero again -- the loop puts the barriers around both),
// count() for one record, whether count() wants the record's strata (STRATA: eval_rec_any<true>), and PERIOD: the turns of the record loop
// after which the counters are merged inside the loop because they could wrap otherwise; 0: only at the end.

// the main table: the window and the floor score's bin in LDS, any other score to the spill list
struct Plain {
    static constexpr int THREADS = EV_THREADS;
    static constexpr uint32_t PERIOD = 0;       // (a block counts far fewer than 2^32 records)
    static constexpr bool STRATA = false;
    uint32_t *h;                                // 5 x (EVAL_WIN + 1)

    __device__ __forceinline__ void zero() const
    {
        for (int i = threadIdx.x; i < 5 * (EVAL_WIN + 1); i += THREADS) h[i] = 0;
    }
    __device__ __forceinline__ void merge(const EvalRecArgs &A) const
    {
        for (int i = threadIdx.x; i < 5 * (EVAL_WIN + 1); i += THREADS) {
            const uint32_t v = h[i];
            if (!v) continue;
            h[i] = 0;
            atomicAdd(&A.hist[i], (unsigned long long)v);
        }
    }
    __device__ __forceinline__ void count(const EvalRecArgs &A, const ev::Rec &, const ev::Out &o, const ev::Strata &) const
    {
        const int64_t bin = (int64_t)o.score - A.win_lo;
        if (bin >= 0 && bin < EVAL_WIN) atomicAdd(&h[o.cls * (EVAL_WIN + 1) + (uint32_t)bin], 1u);
        else if (o.score == A.floor_score) atomicAdd(&h[o.cls * (EVAL_WIN + 1) + EVAL_WIN], 1u);
        else {
            const uint32_t k = atomicAdd(&A.res->n_spill, 1u);
            A.spill[k] = ((uint64_t)(uint32_t)o.score << 32) | (uint32_t)o.cls;
        }
    }
};

// the breakdown: once per selected dimension, in the record's stratum of it; 16-bit counters, two to an LDS word
constexpr int BD_THREADS = 512;
constexpr uint32_t BD_FLUSH_ITERS = 65535u / BD_THREADS;        // a block counts fewer than 2^16 records between two merges
static_assert(BD_FLUSH_ITERS >= 1 && BD_FLUSH_ITERS * BD_THREADS < 65536u, "a 16-bit counter must not wrap between two merges");

struct Breakdown {
    static constexpr int THREADS = BD_THREADS;
    static constexpr uint32_t PERIOD = BD_FLUSH_ITERS;
    static constexpr bool STRATA = true;
    const EvalBdArgs &B;
    uint32_t *h;                                // EVAL_BD_CTRS / 2 words
    uint32_t bins, n_words;                     // bins per (row, class); the words that the selected dimensions' counters take

    __device__ __forceinline__ Breakdown(const EvalBdArgs &b, uint32_t *lds) : B(b), h(lds), bins(b.win + 1), n_words((b.n_rows * 5 * (b.win + 1) + 1) / 2) {}
    __device__ __forceinline__ void zero() const
    {
        for (uint32_t i = threadIdx.x; i < n_words; i += THREADS) h[i] = 0;
    }
    __device__ __forceinline__ void merge(const EvalRecArgs &) const
    {
        for (uint32_t i = threadIdx.x; i < n_words; i += THREADS) {
            const uint32_t v = h[i];
            if (!v) continue;
            h[i] = 0;
            if (v & 0xffffu) atomicAdd(&B.hist[2 * i], (unsigned long long)(v & 0xffffu));
            if (v >> 16) atomicAdd(&B.hist[2 * i + 1], (unsigned long long)(v >> 16));
        }
    }
    // one more record in counter (row * 5 + cls) * (win + 1) + bin
    __device__ __forceinline__ void one(uint32_t row, uint32_t cls, uint32_t bin) const
    {
        const uint32_t k = (row * 5 + cls) * bins + bin;
        if (k < EVAL_BD_CTRS) atomicAdd(&h[k >> 1], 1u << ((k & 1) * 16));
    }
    __device__ __forceinline__ void count(const EvalRecArgs &A, const ev::Rec &, const ev::Out &o, const ev::Strata &sv) const
    {
        const uint32_t s_snps = ev::capped(sv.snps, B.cap), s_errors = ev::capped(sv.errors, B.cap), s_indels = sv.indels ? 1 : 0, s_end = sv.end ? 1 : 0;
        const int64_t d = (int64_t)o.score - B.win_lo;
        if ((d >= 0 && d < (int64_t)B.win) || o.score == A.floor_score) {
            const uint32_t bin = (d >= 0 && d < (int64_t)B.win) ? (uint32_t)d : B.win, cls = (uint32_t)o.cls;
            if (B.row_snps >= 0) one((uint32_t)B.row_snps + s_snps, cls, bin);
            if (B.row_errors >= 0) one((uint32_t)B.row_errors + s_errors, cls, bin);
            if (B.row_indels >= 0) one((uint32_t)B.row_indels + s_indels, cls, bin);
            if (B.row_end >= 0) one((uint32_t)B.row_end + s_end, cls, bin);
        } else {
            const uint32_t k = atomicAdd(&A.res->n_spill, 1u);
            A.spill[k] = ev::bd_spill_pack(o.score, o.cls, s_snps, s_errors, s_indels, s_end);
        }
    }
};

// The truth: Plain's count, and for a mapped record the join of SPEC TRUTH and its counts.  A compared record adds at most TR_LDS_MAX to an LDS
// counter (a longer one goes to the global counters directly), so a block adds less than 2^32 to any of them in TR_FLUSH_ITERS turns of its
// record loop.  Reads of 25 000 bases stay in LDS.
constexpr uint64_t TR_LDS_MAX = 65535;
constexpr uint32_t TR_FLUSH_ITERS = (uint32_t)(0xFFFFFFFFull / (EV_THREADS * TR_LDS_MAX));
static_assert(TR_FLUSH_ITERS >= 1 && (uint64_t)TR_FLUSH_ITERS * EV_THREADS * TR_LDS_MAX <= 0xFFFFFFFFull, "a 32-bit counter must not wrap between two merges");
static_assert(TR_LDS_MAX >= 25000, "ordinary reads are counted in LDS");

struct Truth {
    static constexpr int THREADS = EV_THREADS;
    static constexpr uint32_t PERIOD = TR_FLUSH_ITERS;
    static constexpr bool STRATA = false;
    const EvalTruthArgs &T;
    Plain plain;
    uint32_t *tc;                               // EVAL_TR_CTRS

    __device__ __forceinline__ void zero() const
    {
        plain.zero();
        for (uint32_t i = threadIdx.x; i < EVAL_TR_CTRS; i += THREADS) tc[i] = 0;
    }
    __device__ __forceinline__ void merge(const EvalRecArgs &A) const
    {
        plain.merge(A);
        for (uint32_t i = threadIdx.x; i < EVAL_TR_CTRS; i += THREADS) {
            const uint32_t v = tc[i];
            if (!v) continue;
            tc[i] = 0;
            atomicAdd(&T.ctrs[i], (unsigned long long)v);
        }
    }
    __device__ __forceinline__ void join(const EvalRecArgs &A, const ev::Rec &R, ev::TruthCmp *c) const
    {
        c->outcome = ev::J_MISSING; c->exact = 0; c->indel = false;
        c->bases = c->right = c->clipped = c->ibases = c->iright = 0;
        if (!ev::key_valid(R.flag)) return;
        uint64_t h1, h2;
        ev::key_hash(R.qname, (uint32_t)R.qlen, ev::key_end(R.flag), &h1, &h2);
        const int64_t f = ev::truth_find(T.slots, T.mask, T.recs, h1, h2);
        if (f < 0) return;
        const int32_t t = R.bam ? R.tid : ev::target_find(A.tg, R.rname, R.rname_len);
        ev::truth_compare(R, t >= 0 ? T.tmap[t] : -1, T.recs[f], T.pool, c);
    }
    // in stratum all and, for a compared record of an indel truth, in stratum indel
    __device__ __forceinline__ void count(const EvalRecArgs &A, const ev::Rec &R, const ev::Out &o, const ev::Strata &sv) const
    {
        plain.count(A, R, o, sv);
        if (R.flag & 4) return;
        ev::TruthCmp c;
        join(A, R, &c);
        const uint64_t v[EVAL_TR_COLS] = {c.outcome == ev::J_MISSING, c.outcome == ev::J_RANDOM, c.outcome == ev::J_UNUSABLE, c.outcome == ev::J_COMPARED,
                                          (uint64_t)c.exact, c.bases, c.right, c.clipped, c.ibases, c.iright};
        const bool lds = c.bases <= TR_LDS_MAX;     // (right, clipped, ibases, iright <= bases)
        for (uint32_t s = 0; s < (c.indel ? 2u : 1u); ++s)
            for (uint32_t k = 0; k < EVAL_TR_COLS; ++k) {
                if (!v[k]) continue;
                const uint32_t at = (s * 256 + R.mapq) * EVAL_TR_COLS + k;
                if (lds) atomicAdd(&tc[at], (uint32_t)v[k]);
                else atomicAdd(&T.ctrs[at], (unsigned long long)v[k]);
            }
    }
};

// ---- the record loop ----
// One lane per record.  Block-stride with a guard, so that every lane of a block makes the same number of turns and reaches the barriers of a
// merge inside the loop.  (The form comes by value: by reference the breakdown kernels' frame grew from 80 to 96 bytes of scratch.)
template <class Front, class Form> __device__ __forceinline__ void eval_records_loop(const EvalRecArgs &A, const Form F)
{
    F.zero();
    __syncthreads();

    const uint32_t n_lines = A.res->n_lines;
    const uint32_t n_rec = n_lines > A.has_ctx ? n_lines - A.has_ctx : 0;
    uint32_t n_local = 0;
    [[maybe_unused]] uint32_t turns = 0;
    for (uint64_t base = (uint64_t)blockIdx.x * Form::THREADS; base < n_rec; base += (uint64_t)gridDim.x * Form::THREADS) {
        const uint64_t r64 = base + threadIdx.x;
        if (r64 < n_rec) {
            const uint32_t r = (uint32_t)r64, li = r + A.has_ctx;
            ev::Rec R;
            ev::Out o = {ev::E_MALFORMED, 0, 0, -1, 0};
            ev::Strata sv = {0, 0, 0, 0};
            if (Front::rec(A, li, &R)) {
                ev::Prev pv;
                const bool have_prev = A.opt.m && li;
                if (have_prev) pv = Front::prev(A, li);
                o = ev::eval_rec_any<Form::STRATA>(R, have_prev ? &pv : nullptr, A.opt, A.tg, &sv);
            }
            bool incorrect = false;
            if (o.code) {
                atomicMin((unsigned long long *)&A.res->err, (unsigned long long)(((uint64_t)r << 8) | (uint32_t)o.code));
            } else if (!o.skipped) {
                n_local += (uint32_t)o.n_inc;
                if (o.cls >= 0) {
                    incorrect = o.cls == ev::MI || o.cls == ev::UM;
                    F.count(A, R, o, sv);
                }
            }
            if (A.flags) A.flags[r] = incorrect ? 1 : 0;
        }
        if constexpr (Form::PERIOD != 0) {
            if (++turns == Form::PERIOD) {
                turns = 0;
                __syncthreads();
                F.merge(A);
                __syncthreads();
            }
        }
    }
    if (n_local) atomicAdd((unsigned long long *)&A.res->n, (unsigned long long)n_local);
    __syncthreads();
    F.merge(A);
}

__global__ __launch_bounds__(EV_THREADS) void k_eval_records(EvalRecArgs A)
{
    __shared__ uint32_t h[(EVAL_WIN + 1) * 5];
    eval_records_loop<SamFront>(A, Plain{h});
}

// a BAM chunk: A.ends holds the byte offset of every record of the chunk (host-made: dw_eval.cpp hops over the block_size chain), and
// A.res->n_lines their number; no newline kernels run
__global__ __launch_bounds__(EV_THREADS) void k_eval_bam_records(EvalRecArgs A)
{
    __shared__ uint32_t h[(EVAL_WIN + 1) * 5];
    eval_records_loop<BamFront>(A, Plain{h});
}

__global__ __launch_bounds__(BD_THREADS) void k_eval_records_bd(EvalRecArgs A, EvalBdArgs B)
{
    __shared__ uint32_t hb[EVAL_BD_CTRS / 2];
    eval_records_loop<SamFront>(A, Breakdown(B, hb));
}

__global__ __launch_bounds__(BD_THREADS) void k_eval_bam_records_bd(EvalRecArgs A, EvalBdArgs B)
{
    __shared__ uint32_t hb[EVAL_BD_CTRS / 2];
    eval_records_loop<BamFront>(A, Breakdown(B, hb));
}

__global__ __launch_bounds__(EV_THREADS) void k_eval_records_tr(EvalRecArgs A, EvalTruthArgs T)
{
    __shared__ uint32_t ht[(EVAL_WIN + 1) * 5];
    __shared__ uint32_t tct[EVAL_TR_CTRS];
    eval_records_loop<SamFront>(A, Truth{T, Plain{ht}, tct});
}

__global__ __launch_bounds__(EV_THREADS) void k_eval_bam_records_tr(EvalRecArgs A, EvalTruthArgs T)
{
    __shared__ uint32_t ht[(EVAL_WIN + 1) * 5];
    __shared__ uint32_t tct[EVAL_TR_CTRS];
    eval_records_loop<BamFront>(A, Truth{T, Plain{ht}, tct});
}

// ---- the truth: load and index (dw_eval.hpp TRUTH) ----

// line li of a chunk of truth text
__device__ __forceinline__ const char *truth_line(const EvalTruthLoadArgs &L, uint32_t li, uint32_t *len)
{
    const uint32_t b = li ? L.ends[li - 1] + 1 : 0;
    *len = L.ends[li] - b;
    return (const char *)L.text + b;
}

// every line checked; cnt[li] = the pool words it needs
__global__ __launch_bounds__(EV_THREADS) void k_truth_count(EvalTruthLoadArgs L)
{
    for (uint32_t li = blockIdx.x * EV_THREADS + threadIdx.x; li < L.n_lines; li += gridDim.x * EV_THREADS) {
        uint32_t len;
        const char *p = truth_line(L, li, &len);
        ev::TruthLine t;
        const int code = ev::truth_parse(p, len, L.tg, &t);
        if (code) atomicMin(L.err, (unsigned long long)(((uint64_t)li << 8) | (uint32_t)code));
        L.cnt[li] = (code || t.unmapped || t.one_m) ? 0 : t.n_ops;
    }
}

// the records and their pool words (only after a chunk without a bad line)
__global__ __launch_bounds__(EV_THREADS) void k_truth_write(EvalTruthLoadArgs L)
{
    for (uint32_t li = blockIdx.x * EV_THREADS + threadIdx.x; li < L.n_lines; li += gridDim.x * EV_THREADS) {
        uint32_t len;
        const char *p = truth_line(L, li, &len);
        ev::TruthLine t;
        if (ev::truth_parse(p, len, L.tg, &t)) continue;
        L.recs[li] = ev::truth_pack(p, t, L.pool, L.pool_base + L.cnt[li]);
    }
}

// Insertion with atomicMin alone: the smaller of the entry and the slot's stays, the larger goes on to the next slot, until a slot was empty.
// Slots never become empty again, so every entry stays reachable from its home slot (the table has more slots than records)
__global__ __launch_bounds__(EV_THREADS) void k_truth_insert(unsigned long long *slots, uint32_t mask, const ev::TruthRec *recs, uint32_t n)
{
    for (uint32_t i = blockIdx.x * EV_THREADS + threadIdx.x; i < n; i += gridDim.x * EV_THREADS) {
        unsigned long long e = ev::slot_entry(recs[i].h1, i);
        uint32_t s = ev::slot_home(recs[i].h1, mask);
        for (uint64_t step = 0; step < 2 * ((uint64_t)mask + 1); ++step, s = (s + 1) & mask) {
            const unsigned long long old = atomicMin(&slots[s], e);
            if (old == ev::SLOT_EMPTY) break;
            if (old > e) e = old;
        }
    }
}

// every record looks itself up and must be the first with its 128 bits: err = (record << 32) | the one found instead, of the first that is not
__global__ __launch_bounds__(EV_THREADS) void k_truth_check(const unsigned long long *slots, uint32_t mask, const ev::TruthRec *recs, uint32_t n, unsigned long long *err)
{
    for (uint32_t i = blockIdx.x * EV_THREADS + threadIdx.x; i < n; i += gridDim.x * EV_THREADS) {
        const int64_t f = ev::truth_find(slots, mask, recs, recs[i].h1, recs[i].h2);
        if (f != (int64_t)i) atomicMin(err, (unsigned long long)(((uint64_t)i << 32) | (uint32_t)f));
    }
}

// ---- launchers ----

static uint32_t truth_grid(uint32_t n)
{
    const uint32_t g = (n + EV_THREADS - 1) / EV_THREADS;
    return g < 1 ? 1 : g > 2048 ? 2048 : g;
}

void launch_eval_newlines(hipStream_t st, const uint8_t *text, uint64_t len, uint32_t *tile_count, EvalRes *res, uint32_t *ends)
{
    const uint32_t tiles = (uint32_t)((len + EV_TILE - 1) / EV_TILE);
    if (!tiles) return;
    hipLaunchKernelGGL(k_eval_count, dim3(tiles), dim3(EV_THREADS), 0, st, text, len, tile_count);
    hipLaunchKernelGGL(k_eval_scan, dim3(1), dim3(EV_THREADS), 0, st, tile_count, tiles, res);
    hipLaunchKernelGGL(k_eval_lines, dim3(tiles), dim3(EV_THREADS), 0, st, text, len, (const uint32_t *)tile_count, ends);
}

void launch_truth_load(hipStream_t st, const EvalTruthLoadArgs &L, EvalRes *scan_res)
{
    hipLaunchKernelGGL(k_truth_count, dim3(truth_grid(L.n_lines)), dim3(EV_THREADS), 0, st, L);
    hipLaunchKernelGGL(k_eval_scan, dim3(1), dim3(EV_THREADS), 0, st, L.cnt, L.n_lines, scan_res);
}

void launch_truth_write(hipStream_t st, const EvalTruthLoadArgs &L)
{
    hipLaunchKernelGGL(k_truth_write, dim3(truth_grid(L.n_lines)), dim3(EV_THREADS), 0, st, L);
}

void launch_truth_index(hipStream_t st, unsigned long long *slots, uint32_t mask, const ev::TruthRec *recs, uint32_t n, unsigned long long *err)
{
    hipLaunchKernelGGL(k_truth_insert, dim3(truth_grid(n)), dim3(EV_THREADS), 0, st, slots, mask, recs, n);
    hipLaunchKernelGGL(k_truth_check, dim3(truth_grid(n)), dim3(EV_THREADS), 0, st, (const unsigned long long *)slots, mask, recs, n, err);
}

// The grid of a record kernel for `lanes` lanes of work: at most 1 024 blocks' worth of EV_THREADS lanes, in blocks of the form's size
// (the breakdown form's blocks have twice the lanes, so it gets half the blocks)
static uint32_t form_grid(uint64_t lanes, uint32_t threads)
{
    uint64_t g = (lanes + EV_THREADS - 1) / EV_THREADS;
    g = g < 1 ? 1 : g > 1024 ? 1024 : g;
    return (uint32_t)((g * EV_THREADS + threads - 1) / threads);
}

// the record kernel of a front in the run's form
template <class K, class KB, class KT>
static void launch_records(hipStream_t st, K plain, KB bd, KT tr, uint64_t lanes, const EvalRecArgs &A, const EvalBdArgs *B, const EvalTruthArgs *T)
{
    if (B) hipLaunchKernelGGL(bd, dim3(form_grid(lanes, Breakdown::THREADS)), dim3(Breakdown::THREADS), 0, st, A, *B);
    else if (T) hipLaunchKernelGGL(tr, dim3(form_grid(lanes, Truth::THREADS)), dim3(Truth::THREADS), 0, st, A, *T);
    else hipLaunchKernelGGL(plain, dim3(form_grid(lanes, Plain::THREADS)), dim3(Plain::THREADS), 0, st, A);
}

void launch_eval_chunk(hipStream_t st, const EvalRecArgs &A, const EvalBdArgs *B, const EvalTruthArgs *T, uint64_t len, uint32_t *tile_count)
{
    launch_eval_newlines(st, A.text, len, tile_count, A.res, A.ends);
    launch_records(st, k_eval_records, k_eval_records_bd, k_eval_records_tr, (len + 255) / 256, A, B, T);      // about 256 bytes of text per lane
}

void launch_eval_bam_chunk(hipStream_t st, const EvalRecArgs &A, const EvalBdArgs *B, const EvalTruthArgs *T, uint32_t n_rec)
{
    launch_records(st, k_eval_bam_records, k_eval_bam_records_bd, k_eval_bam_records_tr, n_rec, A, B, T);      // one record per lane
}

} // namespace dw
