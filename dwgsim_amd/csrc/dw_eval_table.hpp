// dw_eval_table.hpp -- host-only text of dwgsim_eval-hip that needs no device: the reference's table (dwgsim_eval.c dwgsim_eval_counts_print),
// the breakdown's dimension list, its counter layout and its sections.  dw_eval.cpp uses it; tests/eval_table_main.cpp runs it alone under the
// address and undefined-behaviour sanitizers.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <array>
#include <map>
#include <string>
#include <vector>
#include "dw_eval.hpp"

namespace dw {
namespace evt {

typedef std::array<uint64_t, 5> Row;            // mc mi mu um uu at one score
typedef std::map<int32_t, Row> Rows;            // score -> counts

// the 19 '#' lines and one row per score from max(0, highest) down to min(0, lowest); no counts at all: one row of zeros at threshold 0
inline std::string table_text(const Rows &rows, int32_t a, int32_t d)
{
    int64_t lo = 0, hi = 0;
    uint64_t total = 0, m_total = 0, u_total = 0;
    for (auto &kv : rows) {
        lo = kv.first < lo ? kv.first : lo;
        hi = kv.first > hi ? kv.first : hi;
        const auto &r = kv.second;
        total += r[0] + r[1] + r[2] + r[3] + r[4];
        m_total += r[0] + r[1] + r[2];
        u_total += r[3] + r[4];
    }
    const int w = total ? (int)(1 + log10((double)total)) : 1;
    std::string t = std::string("# thr | the minimum ") + (a == 0 ? "mapping quality" : "alignment score") + " threshold\n";
    t += "# mc | the number of correctly mapped reads that should be mapped at the threshold\n"
         "# mi | the number of incorrectly mapped reads that should be mapped at the threshold\n"
         "# mu | the number of unmapped reads that should be mapped at the threshold\n"
         "# um | the number of mapped reads that should be unmapped at the threshold\n"
         "# uu | the number of unmapped reads that should be unmapped at the threshold\n"
         "# mc + mi + mu + um + uu | the total number of reads at the threshold\n"
         "# mc' | the number of correctly mapped reads that should be mapped at or greater than that threshold\n"
         "# mi' | the number of incorrectly mapped reads that should be mapped at or greater than that threshold\n"
         "# mu' | the number of unmapped reads that should be mapped at or greater than that threshold\n"
         "# um' | the number of mapped reads that should be unmapped at or greater than that threshold\n"
         "# uu' | the number of unmapped reads that should be unmapped at or greater than that threshold\n"
         "# mc' + mi' + mu' + um' + uu' | the total number of reads at or greater than the threshold\n"
         "# (mc / (mc' + mi' + mu')) | sensitivity: the fraction of mappable reads that are mapped correctly at the threshold\n"
         "# (mc / (mc' + mi')) | positive predictive value: the fraction of mapped mappable reads that are mapped correctly at the threshold\n"
         "# (um / (um' + uu')) | false discovery rate: the fraction of random reads that are mapped at the threshold\n"
         "# (mc' / (mc' + mi' + mu')) | sensitivity: the fraction of mappable reads that are mapped correctly at or greater than the threshold\n"
         "# (mc' / (mc' + mi')) | positive predictive value: the fraction of mapped mappable reads that are mapped correctly at or greater than the threshold\n"
         "# (um' / (um' + uu')) | false discovery rate: the fraction of random reads that are mapped at or greater than the threshold\n";
    uint64_t sum[5] = {0, 0, 0, 0, 0}, mm_total = 0;
    char buf[512];
    const Row zero = {0, 0, 0, 0, 0};
    auto it = rows.rbegin();
    for (int64_t sc = hi; sc >= lo; --sc) {
        while (it != rows.rend() && it->first > sc) ++it;
        const Row &r = (it != rows.rend() && it->first == sc) ? it->second : zero;
        for (int k = 0; k < 5; ++k) sum[k] += r[k];
        mm_total += r[0] + r[1];
        double den = (double)(r[0] + r[1] + r[2]);
        const double sens_at = den == 0 ? 0. : r[0] / den;
        const double sens_ge = m_total == 0 ? 0. : sum[0] / (double)m_total;
        den = (double)(r[0] + r[1]);
        const double ppv_at = den == 0 ? 0. : r[0] / den;
        const double ppv_ge = mm_total == 0 ? 0. : sum[0] / (double)mm_total;
        den = (double)(r[3] + r[4]);
        const double fdr_at = den == 0 ? 0. : r[3] / den;
        const double fdr_ge = u_total == 0 ? 0. : sum[3] / (double)u_total;
        const int32_t thr = (int32_t)((uint32_t)(int32_t)sc * (uint32_t)d);
        int k = snprintf(buf, sizeof buf, "%.2d ", thr);
        const uint64_t v[12] = {r[0], r[1], r[2], r[3], r[4], r[0] + r[1] + r[2] + r[3] + r[4], sum[0], sum[1], sum[2], sum[3], sum[4],
                                sum[0] + sum[1] + sum[2] + sum[3] + sum[4]};
        for (int j = 0; j < 12; ++j) k += snprintf(buf + k, sizeof buf - k, "%*llu ", w, (unsigned long long)v[j]);
        snprintf(buf + k, sizeof buf - k, "%.3e %.3e %.3e %.3e %.3e %.3e\n", sens_at, ppv_at, fdr_at, sens_ge, ppv_ge, fdr_ge);
        t += buf;
    }
    return t;
}

// the window part of a table: counts[cls * (win + 1) + k], bin k < win = score win_lo + k, bin win = floor_score
inline void add_window(Rows &rows, const unsigned long long *counts, uint32_t win, int32_t win_lo, int32_t floor_score)
{
    for (uint32_t k = 0; k <= win; ++k)
        for (int cl = 0; cl < 5; ++cl) {
            const uint64_t v = counts[(size_t)cl * (win + 1) + k];
            if (v) rows[k < win ? (int32_t)(win_lo + (int64_t)k) : floor_score][cl] += v;
        }
}

// ---- breakdown (dw_eval.hpp BREAKDOWN) ----
struct Breakdown {
    bool on = false;
    int cap = ev::BD_DEFAULT_CAP;
    bool sel[ev::N_DIMS] = {false, false, false, false};
    int row[ev::N_DIMS] = {-1, -1, -1, -1};       // the first counter row of a selected dimension
    int n_rows = 0;                               // strata of all selected dimensions
    int first = -1;                               // the first selected dimension: the main table is the sum of its strata
    uint32_t win = 0;                             // scores per row in the kernel's window
    int32_t win_lo = 0;
    size_t counters() const { return ((size_t)n_rows * 5 * (win + 1) + 1) & ~(size_t)1; }
};

inline const char *dim_name(int dim) { return dim == ev::D_SNPS ? "snps" : dim == ev::D_ERRORS ? "errors" : dim == ev::D_INDELS ? "indels" : "end"; }

// dims: a comma list of snps, errors, indels, end (NULL or empty: off); cap 0: the default, else 1 ... 32.  `a`: the run's -a (the window of
// -a 0 starts at score 0, the others a quarter below it).  block_counters: what a block of the kernel holds.  nullptr, or what is wrong.
inline const char *parse_breakdown(const char *dims, int cap, int32_t a, uint32_t block_counters, uint32_t max_win, Breakdown *out)
{
    Breakdown b;
    if (cap < 0 || cap > ev::BD_MAX_CAP) return "breakdown: the cap must be 0 (default) or 1 ... 32";
    b.cap = cap ? cap : ev::BD_DEFAULT_CAP;
    if (!dims || !*dims) { *out = b; return nullptr; }
    for (const char *p = dims;;) {
        const char *e = strchr(p, ',');
        const size_t n = e ? (size_t)(e - p) : strlen(p);
        int dim = -1;
        for (int k = 0; k < ev::N_DIMS; ++k)
            if (strlen(dim_name(k)) == n && !memcmp(dim_name(k), p, n)) dim = k;
        if (dim < 0) return "breakdown: unknown dimension (snps, errors, indels, end)";
        if (b.sel[dim]) return "breakdown: a dimension is named twice";
        b.sel[dim] = true;
        if (!e) break;
        p = e + 1;
    }
    b.on = true;
    for (int k = 0; k < ev::N_DIMS; ++k)
        if (b.sel[k]) {
            if (b.first < 0) b.first = k;
            b.row[k] = b.n_rows;
            b.n_rows += ev::dim_strata(k, b.cap);
        }
    const uint32_t per_row = block_counters / ((uint32_t)b.n_rows * 5);       // at least 93: 70 rows at most
    b.win = per_row - 1 < max_win ? per_row - 1 : max_win;
    b.win_lo = a == 0 ? 0 : -(int32_t)(b.win / 4);
    *out = b;
    return nullptr;
}

// "snps=3", "errors=8+", "indels=1+", "end=2"
inline std::string stratum_label(int dim, int k, int cap)
{
    std::string s = std::string(dim_name(dim)) + "=";
    if (dim == ev::D_END) return s + (k ? "2" : "1");
    if (dim == ev::D_INDELS) return s + (k ? "1+" : "0");
    return s + std::to_string(k) + (k == cap ? "+" : "");
}

// The counts of a breakdown run: the kernel's counters (Breakdown::counters() words) and the decoded spill list
struct BreakdownCounts {
    std::map<std::pair<int, int32_t>, Row> spill;      // (counter row, score) -> counts, of the selected dimensions
    void add_spill(const Breakdown &b, uint64_t word, Rows *main)
    {
        int32_t score; int cls; uint32_t s[ev::N_DIMS];
        ev::bd_spill_unpack(word, &score, &cls, s);
        if (cls > 4) return;
        (*main)[score][cls]++;
        for (int k = 0; k < ev::N_DIMS; ++k)
            if (b.sel[k] && (int)s[k] < ev::dim_strata(k, b.cap)) spill[{b.row[k] + (int)s[k], score}][cls]++;
    }
    Rows rows_of(const Breakdown &b, const unsigned long long *counters, int row, int32_t floor_score) const
    {
        Rows r;
        add_window(r, counters + (size_t)row * 5 * (b.win + 1), b.win, b.win_lo, floor_score);
        for (auto it = spill.lower_bound({row, INT32_MIN}); it != spill.end() && it->first.first == row; ++it)
            for (int cl = 0; cl < 5; ++cl) r[it->first.second][cl] += it->second[cl];
        return r;
    }
};

// the window counts of the main table: the sum of the first selected dimension's strata
inline void add_main_window(const Breakdown &b, const unsigned long long *counters, int32_t floor_score, Rows *main)
{
    for (int k = 0; k < ev::dim_strata(b.first, b.cap); ++k)
        add_window(*main, counters + (size_t)(b.row[b.first] + k) * 5 * (b.win + 1), b.win, b.win_lo, floor_score);
}

// one section per stratum: "## <label>\n" and that stratum's table; dimensions in their fixed order, strata ascending, empty ones included
inline std::string breakdown_text(const Breakdown &b, const BreakdownCounts &c, const unsigned long long *counters, int32_t floor_score, int32_t a, int32_t d)
{
    std::string t;
    for (int dim = 0; dim < ev::N_DIMS; ++dim) {
        if (!b.sel[dim]) continue;
        for (int k = 0; k < ev::dim_strata(dim, b.cap); ++k) {
            t += "## " + stratum_label(dim, k, b.cap) + "\n";
            t += table_text(c.rows_of(b, counters, b.row[dim] + k, floor_score), a, d);
        }
    }
    return t;
}

} // namespace evt
} // namespace dw
