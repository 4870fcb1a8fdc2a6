// tests/bam_inflate_main.cpp -- TEST INFRASTRUCTURE ONLY: a stand-alone program over dw_inflate.hpp and the BGZF framing of dw_bam.hpp, built by
// tests/test_bam_inflate.py with -fsanitize=address,undefined.  It reads a file of cases and runs each one on heap blocks of exactly the
// case's sizes (the sanitizer sees a read past src_len), with a guard region behind dst that it checks itself.
//   case: kind u8, src_len u32, dst_cap u32, exp_len u32, exp_crc u32, src[src_len], expected[exp_len]
//   kind 0  a raw deflate stream that must inflate to `expected`, whose CRC-32 must be exp_crc
//   kind 1  a BGZF block that must frame, and inflate to `expected` with matching CRC-32 and ISIZE (inflate_job)
//   kind 2  a damaged BGZF block: framing and inflating must return, with an error or with some output, never with more than dst_cap bytes
// Prints one line per kind with its counts; exit status 1 and a message on the first case that does not hold.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "dw_bam.hpp"

using namespace dw;

static const size_t GUARD = 64;

static uint32_t rd32(FILE *f)
{
    uint8_t b[4];
    if (fread(b, 1, 4, f) != 4) { fprintf(stderr, "short case file\n"); exit(2); }
    return bam::le32(b);
}

static uint8_t *heap_copy(FILE *f, size_t n)
{
    uint8_t *p = (uint8_t *)malloc(n ? n : 1);
    if (n && fread(p, 1, n, f) != n) { fprintf(stderr, "short case file\n"); exit(2); }
    return p;
}

// inflate into a block of dst_cap bytes plus the guard; -100 when the guard was touched or more than dst_cap bytes are reported
static int guarded_inflate(const uint8_t *src, size_t src_len, size_t dst_cap, std::vector<uint8_t> *out)
{
    uint8_t *dst = (uint8_t *)malloc(dst_cap + GUARD);
    memset(dst + dst_cap, 0xA5, GUARD);
    size_t got = ~(size_t)0;
    const int r = zz::inflate(src, src_len, dst, dst_cap, &got);
    bool ok = got <= dst_cap;
    for (size_t i = 0; i < GUARD; ++i) ok = ok && dst[dst_cap + i] == 0xA5;
    if (ok && out) out->assign(dst, dst + got);
    free(dst);
    return ok ? r : -100;
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: bam_inflate_main CASES\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    long n_case = 0, count[3] = {0, 0, 0}, damaged_err = 0, damaged_out = 0;
    for (int kind; (kind = fgetc(f)) != EOF; ++n_case) {
        const uint32_t src_len = rd32(f), dst_cap = rd32(f), exp_len = rd32(f), exp_crc = rd32(f);
        uint8_t *src = heap_copy(f, src_len), *expected = heap_copy(f, exp_len);
        std::vector<uint8_t> out;
        auto fail = [&](const char *what) { fprintf(stderr, "case %ld (kind %d): %s\n", n_case, kind, what); exit(1); };
        if (kind < 0 || kind > 2) fail("unknown kind");
        count[kind]++;
        if (kind == 0) {
            const int r = guarded_inflate(src, src_len, dst_cap, &out);
            if (r) fail(r == -100 ? "wrote past dst_cap" : zz::error_name(r));
            if (out.size() != exp_len || (exp_len && memcmp(out.data(), expected, exp_len))) fail("output differs");
            if (zz::crc32(out.data(), out.size()) != exp_crc) fail("CRC-32 differs");
            // the same stream into a block that is one byte short must be refused, not overrun
            if (exp_len && guarded_inflate(src, src_len, exp_len - 1, nullptr) != zz::Z_E_ROOM) fail("a short dst was not refused");
            // and every proper prefix of the stream ends early
            if (src_len && guarded_inflate(src, src_len - 1, dst_cap, nullptr) == -100) fail("wrote past dst_cap on a cut stream");
        } else {
            bam::BgzfBlock b;
            const char *why = nullptr;
            // the framing sees fewer bytes first: it must ask for more, never read past them
            for (size_t cut = 0; cut < src_len && cut < 40; ++cut) {
                uint8_t *part = (uint8_t *)malloc(cut ? cut : 1);
                memcpy(part, src, cut);
                const int k = bam::bgzf_block_at(part, cut, &b, &why);
                free(part);
                if (kind == 1 && k != 0) fail("framing did not wait for the whole block");
            }
            const int k = bam::bgzf_block_at(src, src_len, &b, &why);
            if (kind == 1) {
                if (k != 1 || b.size != src_len) fail("block does not frame");
                std::vector<uint8_t> dst(b.isize + GUARD, 0xA5);
                bam::InflateJob j = {src + b.data_off, b.data_len, dst.data(), b.isize, b.crc, nullptr};
                bam::inflate_job(j);
                if (j.error) fail(j.error);
                for (size_t i = 0; i < GUARD; ++i) if (dst[b.isize + i] != 0xA5) fail("wrote past ISIZE");
                if (b.isize != exp_len || b.crc != exp_crc || (exp_len && memcmp(dst.data(), expected, exp_len))) fail("output differs");
            } else {
                if (k == 1) {
                    if (b.data_off + b.data_len + 8 > src_len) fail("framing accepted a block larger than its bytes");
                    const int r = guarded_inflate(src + b.data_off, b.data_len, dst_cap, &out);
                    if (r == -100) fail("wrote past dst_cap");
                    const bool good = !r && out.size() == b.isize && zz::crc32(out.data(), out.size()) == b.crc;
                    if (good && (out.size() != exp_len || memcmp(out.data(), expected, exp_len))) ++damaged_out;      // (damage that CRC-32 cannot see: counted)
                    if (!good) ++damaged_err;
                } else {
                    ++damaged_err;
                }
                // the bytes behind a BGZF header of the usual size, whatever the framing said
                if (src_len > 18 && guarded_inflate(src + 18, src_len - 18, dst_cap, nullptr) == -100) fail("wrote past dst_cap");
            }
        }
        free(src); free(expected);
    }
    fclose(f);
    printf("raw %ld\nbgzf %ld\ndamaged %ld refused %ld undetected %ld\n", count[0], count[1], count[2], damaged_err, damaged_out);
    return 0;
}
