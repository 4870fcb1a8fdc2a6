// tests/eval_table_main.cpp -- TEST INFRASTRUCTURE ONLY: a stand-alone program over dw_eval_table.hpp (the dimension list of a breakdown, its
// counter layout, the decoding of its spill words, the tables and sections), built by tests/test_eval_table.py with
// -fsanitize=address,undefined.  It reads one case from the file named on its command line:
//   line 1: <dims or -> <cap> <a> <d> <block counters> <max window>
//   then one line per record that enters the table: <score> <class> <n_sub_1> <n_err_1> <own-end indel flag> <end 0|1>
// A record is counted as the kernel counts it: in the window's counters (heap blocks of exactly Breakdown::counters() words, so that the
// sanitizer sees an index past them) or, outside the window, as one ev::bd_spill_pack word that BreakdownCounts decodes.  Output: "error: <why>"
// for a refused dimension list; else the window line, the main table and the sections.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "dw_eval_table.hpp"

using namespace dw;

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: eval_table_main CASE\n"); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    char dims[256];
    int cap, a, d;
    unsigned block_counters, max_win;
    if (fscanf(f, "%255s %d %d %d %u %u", dims, &cap, &a, &d, &block_counters, &max_win) != 6) { fprintf(stderr, "bad case head\n"); return 2; }
    evt::Breakdown b;
    if (const char *why = evt::parse_breakdown(strcmp(dims, "-") ? dims : nullptr, cap, a, block_counters, max_win, &b)) {
        printf("error: %s\n", why);
        return 0;
    }
    int32_t floor_score = ev::cdiv(ev::MINAS, d);
    if (floor_score < ev::MINAS) floor_score = ev::MINAS;
    const size_t n = b.on ? b.counters() : 0;
    unsigned long long *counters = (unsigned long long *)calloc(n ? n : 1, sizeof(unsigned long long));
    evt::BreakdownCounts bc;
    evt::Rows main_spill;
    long long score;
    int cls, snps, errors, indels, end;
    while (fscanf(f, "%lld %d %d %d %d %d", &score, &cls, &snps, &errors, &indels, &end) == 6) {
        if (!b.on) { main_spill[(int32_t)score][cls]++; continue; }
        const uint32_t s[ev::N_DIMS] = {ev::capped(snps, b.cap), ev::capped(errors, b.cap), indels ? 1u : 0u, end ? 1u : 0u};
        const int64_t k = score - b.win_lo;
        if ((k >= 0 && k < (int64_t)b.win) || (int32_t)score == floor_score) {
            const uint32_t bin = (k >= 0 && k < (int64_t)b.win) ? (uint32_t)k : b.win;
            for (int dim = 0; dim < ev::N_DIMS; ++dim)
                if (b.sel[dim]) counters[((size_t)(b.row[dim] + s[dim]) * 5 + cls) * (b.win + 1) + bin]++;
        } else {
            bc.add_spill(b, ev::bd_spill_pack((int32_t)score, cls, s[0], s[1], s[2], s[3]), &main_spill);
        }
    }
    fclose(f);
    printf("window %u %d rows %d\n", b.win, b.win_lo, b.n_rows);
    evt::Rows rows = main_spill;
    if (b.on) evt::add_main_window(b, counters, floor_score, &rows);
    const std::string table = evt::table_text(rows, a, d);
    fwrite(table.data(), 1, table.size(), stdout);
    if (b.on) {
        const std::string text = evt::breakdown_text(b, bc, counters, floor_score, a, d);
        fwrite(text.data(), 1, text.size(), stdout);
    }
    free(counters);
    return 0;
}
