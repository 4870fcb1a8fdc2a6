// dw_eval_launch.hpp -- what dw_eval.cpp hands the kernels of dw_eval.hip
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dw_eval.hpp"

namespace dw {

constexpr uint32_t EVAL_TILE = 4096;      // text bytes per block of the newline kernels
constexpr int EVAL_WIN = 2048;            // scores held in LDS per class (plus one bin for the floor score)

// per chunk, device-written
struct EvalRes {
    unsigned long long err;     // (record << 8) | code of the first fatal record, ~0 when none
    unsigned long long n;       // the n of the reference (pairs or single-end reads)
    uint32_t n_lines;           // lines (BAM: records, set by the host) of the chunk, context line included
    uint32_t n_spill;           // entries of the spill list
};

struct EvalRecArgs {
    const uint8_t *text;
    uint32_t *ends;             // SAM: the position of every newline (device-made).  BAM: the offset of every record (host-made)
    EvalRes *res;
    unsigned long long *hist;   // 5 x (EVAL_WIN + 1): class-major; bin EVAL_WIN of a class = floor_score
    uint64_t *spill;            // (uint32 score << 32) | class
    uint8_t *flags;             // nullptr, or per record: 1 = mapped incorrectly (-p)
    uint32_t has_ctx;
    int32_t win_lo;             // bin k of the window = score win_lo + k
    int32_t floor_score;
    ev::Opts opt;
    ev::Targets tg;
};

// The breakdown form (dw_eval.hpp BREAKDOWN) counts every record once per selected dimension, in that dimension's stratum, instead of once in
// A.hist.  Counter ((row_d + stratum) * 5 + class) * (win + 1) + bin: bin k < win = score win_lo + k, bin win = floor_score.  The host chooses win
// so that all counters of the selected dimensions fit into the block's EVAL_BD_CTRS 16-bit LDS counters; the main table is the sum of the first
// selected dimension's strata.  A score outside the window goes to A.spill as one ev::bd_spill_pack word.  A.hist and A.win_lo are not read.
constexpr uint32_t EVAL_BD_CTRS = 32768;          // 16-bit counters per block: 64 KiB of LDS

struct EvalBdArgs {
    unsigned long long *hist;   // n_rows * 5 * (win + 1) counters, rounded up to an even number
    uint32_t n_rows;            // strata of all selected dimensions
    uint32_t win;
    int32_t win_lo;
    int32_t cap;
    int32_t row_snps, row_errors, row_indels, row_end;      // the first row of each dimension, -1: not selected
};

// The truth form (dw_eval.hpp TRUTH).  Load, per chunk of truth text behind the newline kernels: k_truth_count (every line checked, its pool
// words counted), k_eval_scan over the counts, k_truth_write (records and pool words).  Commit: k_truth_insert, k_truth_check.  Afterwards the
// table, the records and the pool are read-only, and k_eval_records_tr / k_eval_bam_records_tr join every participating record with them.
// Counter (stratum * 256 + MAPQ) * EVAL_TR_COLS + column; stratum 0 all, 1 indel.
enum { TC_MISSING = 0, TC_RANDOM, TC_UNUSABLE, TC_COMPARED, TC_EXACT, TC_BASES, TC_RIGHT, TC_CLIPPED, TC_IBASES, TC_IRIGHT, EVAL_TR_COLS };
constexpr uint32_t EVAL_TR_CTRS = 2 * 256 * EVAL_TR_COLS;       // 32-bit LDS counters per block: 20 KiB

struct EvalTruthLoadArgs {
    const uint8_t *text;
    const uint32_t *ends;           // the position of every newline of the chunk
    uint32_t n_lines;               // (device-made, read back by the host)
    uint32_t *cnt;                  // per line: its pool words; after the scan, where they start within the chunk's
    ev::Targets tg;                 // the truth's own contigs
    ev::TruthRec *recs;             // the chunk's first record
    uint32_t *pool;
    uint32_t pool_base;             // pool words of the chunks before
    unsigned long long *err;        // (line << 8) | T_E_* of the first bad line, ~0 when none
};

struct EvalTruthArgs {
    const unsigned long long *slots;
    uint32_t mask;
    const ev::TruthRec *recs;
    const uint32_t *pool;
    const int32_t *tmap;            // per target of the current file: the truth contig of the same name, or -1
    unsigned long long *ctrs;       // EVAL_TR_CTRS
};

void launch_truth_load(hipStream_t st, const EvalTruthLoadArgs &L, EvalRes *scan_res);
void launch_truth_write(hipStream_t st, const EvalTruthLoadArgs &L);
void launch_truth_index(hipStream_t st, unsigned long long *slots, uint32_t mask, const ev::TruthRec *recs, uint32_t n, unsigned long long *err);
// the newline kernels alone (the truth load runs them before it knows how many records to make room for)
void launch_eval_newlines(hipStream_t st, const uint8_t *text, uint64_t len, uint32_t *tile_count, EvalRes *res, uint32_t *ends);

// One chunk through the record loop.  SAM: `len` bytes of whole lines at A.text, the newline kernels first.  BAM: `n_rec` whole records (the
// context record not counted) whose offsets are at A.ends.  The form: B for a breakdown, else T for a truth, else (both null) plain; the
// kernel's grid follows from len / n_rec and the form's block size, which only dw_eval.hip knows.
void launch_eval_chunk(hipStream_t st, const EvalRecArgs &A, const EvalBdArgs *B, const EvalTruthArgs *T, uint64_t len, uint32_t *tile_count);
void launch_eval_bam_chunk(hipStream_t st, const EvalRecArgs &A, const EvalBdArgs *B, const EvalTruthArgs *T, uint32_t n_rec);

} // namespace dw
