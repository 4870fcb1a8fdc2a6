// dwgsim_eval-hip -- the dwgsim_eval command line (reference src/dwgsim_eval.c main / run) over the dwgsim_hip_eval_* C-ABI.
// Input is BAM unless -S is given, as for the reference.  Without -S the first two bytes of every input are read before a device is opened:
// when one of them is not gzip's 1f 8b the input is text, and the message that asks for -S is printed.
// -B LIST and -K INT are this program's own (both letters are free in the reference's option string): the breakdown's sections follow the table.
// -T FILE, also this program's own: the truth SAM of dwgsim-hip, plain or gzip, read completely before the first alignment file; the base-level
// section (dw_eval.hpp TRUTH) follows the table.  A gzip truth is inflated member by member with dw_inflate.hpp on this one thread.
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include <string>
#include <vector>
#include "../../include/dwgsim_hip.h"
#include "dw_inflate.hpp"

#define PACKAGE_VERSION "0.1.17-hip"

static const char *tf(int v) { return v == 1 ? "True" : "False"; }

static int print_usage(const dwgsim_hip_eval_opts_t *a)
{
    FILE *f = stderr;
    fprintf(f, "\n");
    fprintf(f, "Program: dwgsim_eval-hip (short read simulation evaluator, MI355X hot path of dwgsim_eval)\n");
    fprintf(f, "Version: %s\n", PACKAGE_VERSION);
    fprintf(f, "Contact: Nils Homer <dnaa-help@lists.sourceforge.net>\n\n");
    fprintf(f, "Usage: dwgsim_eval-hip [options] <in.bam> [<in2.bam> ...]   or   -S <in.sam> [<in2.sam> ...]   (- reads stdin)\n\n");
    fprintf(f, "Options:\n");
    fprintf(f, "\t-a\tINT\tsplit by [%d]:\n", a->a);
    fprintf(f, "\t\t\t\t\t0: by mapping quality\n");
    fprintf(f, "\t\t\t\t\t1: by alignment score\n");
    fprintf(f, "\t\t\t\t\t2: by suboptimal alignment score\n");
    fprintf(f, "\t\t\t\t\t3: by alignment score - suboptimal alignment score\n");
    fprintf(f, "\t-b\t\talignments are from BWA (for SOLiD data only) [%s]\n", tf(a->b));
    fprintf(f, "\t-c\t\tcolor space alignments [%s]\n", tf(a->c));
    fprintf(f, "\t-d\tINT\tdivide quality/alignment score by this factor [%d]\n", a->d);
    fprintf(f, "\t-g\t\tgap \"wiggle\" [%d]\n", a->g);
    fprintf(f, "\t-m\t\tconsecutive alignments with the same name (and end for multi-ends) should be treated as multi-mapped reads [%s]\n", tf(a->m));
    fprintf(f, "\t-n\tINT\tnumber of raw input paired-end reads (otherwise, inferred from all SAM records present) [%d]\n", a->n);
    fprintf(f, "\t-q\tINT\tconsider only alignments with this mapping quality or greater [%d]\n", a->q);
    fprintf(f, "\t-z\t\tinput contains only single end reads [%s]\n", tf(a->z));
    fprintf(f, "\t-S\t\tinput is SAM (default: BAM) [%s]\n", tf(0));
    fprintf(f, "\t-p\t\tprint incorrect alignments [%s]\n", tf(a->p));
    fprintf(f, "\t-s\tINT\tconsider only alignments with the number of specified SNPs [%d]\n", a->s);
    fprintf(f, "\t-e\tINT\tconsider only alignments with the number of specified errors [%d]\n", a->e);
    fprintf(f, "\t-i\t\tconsider only alignments with indels [%s]\n", tf(a->i));
    fprintf(f, "\t-P\tSTRING\ta read prefix that was prepended to each read name [%s]\n", a->P ? a->P : "not using");
    fprintf(f, "\t-B\tLIST\talso print the table of every stratum of these dimensions, comma separated: snps,errors,indels,end [%s]\n", "not using");
    fprintf(f, "\t-K\tINT\twith -B: snps and errors have the strata 0 ... INT-1 and INT+ (1 to 32; 0: the default) [%d]\n", 8);
    fprintf(f, "\t-T\tFILE\tthe truth SAM of dwgsim-hip (plain or gzip; not with -B): also print how many bases were placed right [%s]\n", "not using");
    fprintf(f, "\t-h\t\tprint this help message\n");
    return 1;
}

static const char BREAK_LINE[] = "************************************************************\n";

// one file: its '@' lines go to the header call, the rest is fed as it is read
static int run_file(dwgsim_hip_eval_ctx_t *ctx, FILE *in)
{
    std::vector<char> buf(8u << 20);
    std::string header;
    bool in_header = true, at_line_start = true;
    size_t got;
    while ((got = fread(buf.data(), 1, buf.size(), in)) > 0) {
        size_t p = 0;
        if (in_header) {
            while (p < got && in_header) {
                if (at_line_start && buf[p] != '@') { in_header = false; break; }
                const char *nl = (const char *)memchr(buf.data() + p, '\n', got - p);
                const size_t e = nl ? (size_t)(nl - buf.data()) + 1 : got;
                header.append(buf.data() + p, e - p);
                at_line_start = nl != nullptr;
                p = e;
            }
            if (in_header) continue;
            const int r = dwgsim_hip_eval_header(ctx, header.data(), header.size());
            if (r) return r;
        }
        const int r = dwgsim_hip_eval_feed(ctx, buf.data() + p, got - p);
        if (r) return r;
    }
    if (in_header) return dwgsim_hip_eval_header(ctx, header.data(), header.size());
    return DWGSIM_HIP_OK;
}

// the truth SAM: its '@' lines go to the truth header call, the rest is fed as it comes, then the index is built.  0, or 1 after a message
static int load_truth(dwgsim_hip_eval_ctx_t *ctx, const char *path)
{
    FILE *in = fopen(path, "rb");
    if (!in) {
        fprintf(stderr, "dwgsim_eval-hip: -T %s: %s\n", path, strerror(errno));
        return 1;
    }
    std::vector<uint8_t> z;
    std::vector<uint8_t> buf(8u << 20);
    size_t got;
    while ((got = fread(buf.data(), 1, buf.size(), in)) > 0) z.insert(z.end(), buf.begin(), buf.begin() + (ptrdiff_t)got);
    fclose(in);
    std::string header;
    bool in_header = true, at_line_start = true;
    int r = DWGSIM_HIP_OK;
    auto take = [&](const char *t, size_t n) {
        size_t p = 0;
        while (p < n && in_header) {
            if (at_line_start && t[p] != '@') {
                in_header = false;
                r = dwgsim_hip_eval_truth_header(ctx, header.data(), header.size());
                break;
            }
            const char *nl = (const char *)memchr(t + p, '\n', n - p);
            const size_t e = nl ? (size_t)(nl - t) + 1 : n;
            header.append(t + p, e - p);
            at_line_start = nl != nullptr;
            p = e;
        }
        if (!r && p < n) r = dwgsim_hip_eval_truth_feed(ctx, t + p, n - p);
        return r == DWGSIM_HIP_OK;
    };
    if (z.size() >= 2 && z[0] == 0x1f && z[1] == 0x8b) {
        size_t at = 0;
        while (at < z.size()) {
            size_t out_len = 0, member = 0;
            const char *why = nullptr;
            int k;
            while ((k = dw::zz::gzip_member(z.data() + at, z.size() - at, buf.data(), buf.size(), &out_len, &member, &why)) == dw::zz::Z_E_ROOM &&
                   buf.size() / 1100 <= z.size() - at)       // (deflate expands at most 1032 times)
                buf.resize(buf.size() * 2);
            if (k) {
                fprintf(stderr, "dwgsim_eval-hip: -T %s: %s in the gzip member at byte %zu\n", path, why, at);
                return 1;
            }
            if (!take((const char *)buf.data(), out_len)) break;
            at += member;
        }
    } else {
        take((const char *)z.data(), z.size());
    }
    if (!r && in_header) r = dwgsim_hip_eval_truth_header(ctx, header.data(), header.size());
    if (!r) r = dwgsim_hip_eval_truth_commit(ctx);
    if (r) {
        fprintf(stderr, "dwgsim_eval-hip: -T %s: %s\n", path, dwgsim_hip_eval_last_error(ctx));
        return 1;
    }
    return 0;
}

// one BAM file: `lead` (the bytes already read from it), then the rest, as they come
static int run_bam_file(dwgsim_hip_eval_ctx_t *ctx, FILE *in, const std::string &lead)
{
    int r = dwgsim_hip_eval_bam_begin(ctx);
    if (r) return r;
    if ((r = dwgsim_hip_eval_feed_bam(ctx, lead.data(), lead.size()))) return r;
    std::vector<char> buf(8u << 20);
    size_t got;
    while ((got = fread(buf.data(), 1, buf.size(), in)) > 0)
        if ((r = dwgsim_hip_eval_feed_bam(ctx, buf.data(), got))) return r;
    return DWGSIM_HIP_OK;
}

static void open_error(const char *path, int e)
{
    fprintf(stderr, "%s\rIn function \"run\": Fatal Error[OpenFileError]. Variable/Value: %s.\nMessage: Could not open file for reading.\n", BREAK_LINE, path);
    fprintf(stderr, "The file stream error was:: %s\n ***** Exiting due to errors *****\n%s", strerror(e), BREAK_LINE);
}

int main(int argc, char *argv[])
{
    dwgsim_hip_eval_opts_t o;
    dwgsim_hip_eval_opts_default(&o);
    int S = 0;
    std::string P;
    const char *T = nullptr;      // -T: the truth SAM
    const char *B = nullptr;      // -B, -K: the breakdown (dwgsim_hip_eval_set_breakdown)
    int K = 0;
    bool have_K = false;
    const char *chunk = getenv("DWGSIM_EVAL_CHUNK");      // text bytes per device chunk (tests use small ones)
    if (chunk) o.chunk_bytes = strtoull(chunk, nullptr, 10);
    const char *threads = getenv("DWGSIM_EVAL_THREADS");  // host threads that inflate BAM input
    if (threads) o.inflate_threads = atoi(threads);
    int c;
    while ((c = getopt(argc, argv, "a:d:e:g:m:n:q:s:bchimpzSP:B:K:T:")) >= 0) {
        switch (c) {
        case 'a': o.a = atoi(optarg); break;
        case 'b': o.b = 1; break;
        case 'c': o.c = 1; break;
        case 'd': o.d = atoi(optarg); break;
        case 'g': o.g = atoi(optarg); break;
        case 'm': o.m = 1; break;         // "m:" in the reference's option string: -m takes (and ignores) an argument
        case 'h': return print_usage(&o);
        case 'n': o.n = atoi(optarg); break;
        case 'q': o.q = atoi(optarg); break;
        case 'z': o.z = 1; break;
        case 'S': S = 1; break;
        case 'p': o.p = 1; break;
        case 's': o.s = atoi(optarg); break;
        case 'e': o.e = atoi(optarg); break;
        case 'i': o.i = 1; break;
        case 'P': P = optarg; o.P = P.c_str(); break;
        case 'B': B = optarg; break;
        case 'T': T = optarg; break;
        case 'K': {
            char *end = nullptr;
            const long v = strtol(optarg, &end, 10);
            if (end == optarg || *end || v < 0 || v > 32) {
                fprintf(stderr, "dwgsim_eval-hip: -K must be a number from 0 (the default of 8) to 32\n");
                return 1;
            }
            K = (int)v; have_K = true;
            break;
        }
        default: fprintf(stderr, "Unrecognized option: -%c\n", c); return 1;
        }
    }
    if (argc == optind) return print_usage(&o);
    if (have_K && !B) {
        fprintf(stderr, "dwgsim_eval-hip: -K has a meaning only with -B\n");
        return 1;
    }
    if (T && B) {
        fprintf(stderr, "dwgsim_eval-hip: -T and -B cannot be used together\n");
        return 1;
    }
    // BAM: every input is opened and its first two bytes are kept
    std::vector<FILE *> files;
    std::vector<std::string> leads;
    std::vector<int> open_errno;
    if (!S) {
        bool text = false, std_in = false;
        for (int i = optind; i < argc; ++i) {
            const bool is_stdin = !strcmp(argv[i], "-");
            FILE *in = is_stdin ? (std_in ? nullptr : stdin) : fopen(argv[i], "rb");
            open_errno.push_back(in ? 0 : is_stdin ? EBADF : errno);
            std_in |= is_stdin;
            char two[2];
            const size_t got = in ? fread(two, 1, 2, in) : 0;
            files.push_back(in);
            leads.emplace_back(two, got);
            // (a file that cannot be opened is reported in its turn, as with -S)
            if ((in || is_stdin) && !(got == 2 && (unsigned char)two[0] == 0x1f && (unsigned char)two[1] == 0x8b)) text = true;
        }
        if (text) {
            fprintf(stderr, "dwgsim_eval-hip: only SAM text is supported: pass -S (samtools view -h in.bam | dwgsim_eval-hip -S -)\n");
            return 1;
        }
    }
    if (o.d == 0) {
        fprintf(stderr, "dwgsim_eval-hip: -d must not be 0\n");
        return 1;
    }
    int err = 0;
    dwgsim_hip_eval_ctx_t *ctx = dwgsim_hip_eval_create(&o, 0, &err);
    if (!ctx) {
        fprintf(stderr, "dwgsim_eval-hip: cannot start the evaluator on device 0 (error %d)\n", err);
        return 1;
    }
    if (B && dwgsim_hip_eval_set_breakdown(ctx, B, K) != DWGSIM_HIP_OK) {
        fprintf(stderr, "dwgsim_eval-hip: -B / -K: %s\n", dwgsim_hip_eval_last_error(ctx));
        dwgsim_hip_eval_destroy(ctx);
        return 1;
    }
    if (T && load_truth(ctx, T)) {
        dwgsim_hip_eval_destroy(ctx);
        return 1;
    }
    fputs("Analyzing...\nCurrently on:\n0", stderr);
    int r = DWGSIM_HIP_OK;
    for (int i = optind; i < argc && r == DWGSIM_HIP_OK; ++i) {
        if (!S) {
            FILE *in = files[i - optind];
            if (!in) {
                open_error(argv[i], open_errno[i - optind]);
                dwgsim_hip_eval_destroy(ctx);
                return 1;
            }
            r = run_bam_file(ctx, in, leads[i - optind]);
            if (in != stdin) fclose(in);
            continue;
        }
        FILE *in = strcmp(argv[i], "-") ? fopen(argv[i], "rb") : stdin;
        if (!in) {
            open_error(argv[i], errno);
            dwgsim_hip_eval_destroy(ctx);
            return 1;
        }
        r = run_file(ctx, in);
        if (in != stdin) fclose(in);
    }
    if (r != DWGSIM_HIP_OK && r != DWGSIM_HIP_EVAL_STOPPED) {
        fprintf(stderr, "\ndwgsim_eval-hip: %s\n", dwgsim_hip_eval_last_error(ctx));
        dwgsim_hip_eval_destroy(ctx);
        return 1;
    }
    dwgsim_hip_eval_summary_t sm;
    memset(&sm, 0, sizeof sm);
    sm.size = sizeof sm;
    if (dwgsim_hip_eval_finish(ctx, &sm) != DWGSIM_HIP_OK) {
        fprintf(stderr, "\ndwgsim_eval-hip: %s\n", dwgsim_hip_eval_last_error(ctx));
        dwgsim_hip_eval_destroy(ctx);
        return 1;
    }
    // the reference's stderr, minus the "Analyzing..." lines written above
    const size_t skip = strlen("Analyzing...\nCurrently on:\n0");
    if (sm.status == 0) {
        const char *t;
        size_t n;
        if (o.p && dwgsim_hip_eval_incorrect_text(ctx, &t, &n) == DWGSIM_HIP_OK) fwrite(t, 1, n, stdout);
        if (dwgsim_hip_eval_table_text(ctx, &t, &n) == DWGSIM_HIP_OK) fwrite(t, 1, n, stdout);
        if (B && dwgsim_hip_eval_breakdown_text(ctx, &t, &n) == DWGSIM_HIP_OK) fwrite(t, 1, n, stdout);
        if (T && dwgsim_hip_eval_truth_text(ctx, &t, &n) == DWGSIM_HIP_OK) fwrite(t, 1, n, stdout);
        fflush(stdout);
    }
    fwrite(sm.stderr_text + skip, 1, sm.stderr_len - skip, stderr);
    const int status = sm.status;
    dwgsim_hip_eval_destroy(ctx);
    return status;
}
