// tests/eval_truth_main.cpp -- TEST INFRASTRUCTURE ONLY: a stand-alone program over the host side of dwgsim_eval-hip's truth section, built by
// tests/test_eval_truth_model.py with -fsanitize=address,undefined.
//   eval_truth_main gz GZ PLAIN   the gzip members of GZ (dw_inflate.hpp gzip_member, as dwgsim_eval-hip -T reads them) must inflate to the
//                                 bytes of PLAIN; every cut of GZ's last 64 bytes, and a flipped byte in its middle, must be refused or end
//                                 early, never read or write outside the heap blocks of exactly the sizes given
//   eval_truth_main cmp CASES     CASES: a first line "contigs<TAB>name..." (the truth's), then per case one line of three parts separated by
//                                 '|': a truth SAM line, an aligned SAM line, and "<contig index> <n_ref> <hex of the same record in BAM>".
//                                 Prints per case: outcome bases right clipped ibases iright exact indel, from ev::truth_compare over the
//                                 SAM front; the BAM front must give the same.  The pool is a heap block of exactly the record's words.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "dw_eval.hpp"
#include "dw_inflate.hpp"

using namespace dw;

static std::vector<uint8_t> slurp(const char *path)
{
    FILE *f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    std::vector<uint8_t> out;
    uint8_t buf[65536];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + got);
    fclose(f);
    return out;
}

// all members of z[0, n), each from a heap copy of exactly the bytes left into a heap block of exactly cap bytes; false and *why when one fails
static bool gunzip(const uint8_t *z, size_t n, std::vector<uint8_t> *out, const char **why)
{
    size_t at = 0;
    while (at < n) {
        uint8_t *src = (uint8_t *)malloc(n - at);
        memcpy(src, z + at, n - at);
        size_t cap = 1024, got = 0, member = 0;
        int k;
        for (;;) {
            uint8_t *dst = (uint8_t *)malloc(cap);
            k = zz::gzip_member(src, n - at, dst, cap, &got, &member, why);
            if (k == zz::Z_OK) out->insert(out->end(), dst, dst + got);
            free(dst);
            if (k != zz::Z_E_ROOM || cap > (64u << 20)) break;
            cap *= 2;
        }
        free(src);
        if (k) return false;
        at += member;
    }
    return true;
}

static int run_gz(const char *gz_path, const char *plain_path)
{
    const std::vector<uint8_t> z = slurp(gz_path), plain = slurp(plain_path);
    std::vector<uint8_t> out;
    const char *why = "";
    if (!gunzip(z.data(), z.size(), &out, &why)) { fprintf(stderr, "gz: %s\n", why); return 1; }
    if (out != plain) { fprintf(stderr, "gz: output differs (%zu bytes, %zu expected)\n", out.size(), plain.size()); return 1; }
    long refused = 0;
    for (size_t cut = 1; cut <= 64 && cut < z.size(); ++cut) {
        out.clear();
        if (gunzip(z.data(), z.size() - cut, &out, &why)) { fprintf(stderr, "gz: a file cut by %zu bytes was accepted\n", cut); return 1; }
        ++refused;
    }
    std::vector<uint8_t> bad = z;
    bad[bad.size() / 2] ^= 0x5a;
    out.clear();
    const bool ok = gunzip(bad.data(), bad.size(), &out, &why);
    if (ok && out == plain) { fprintf(stderr, "gz: a flipped byte went unnoticed\n"); return 1; }
    printf("gz ok %zu bytes, %ld cuts refused\n", plain.size(), refused);
    return 0;
}

static std::vector<std::string> split(const std::string &s, char sep)
{
    std::vector<std::string> out(1);
    for (char c : s) if (c == sep) out.emplace_back(); else out.back() += c;
    return out;
}

static void print(const ev::TruthCmp &c)
{
    static const char *name[] = {"missing", "random", "unusable", "compared"};
    printf("%s %llu %llu %llu %llu %llu %d %d\n", name[c.outcome], (unsigned long long)c.bases, (unsigned long long)c.right, (unsigned long long)c.clipped,
           (unsigned long long)c.ibases, (unsigned long long)c.iright, c.exact, c.indel ? 1 : 0);
}

static int run_cmp(const char *path)
{
    const std::vector<uint8_t> bytes = slurp(path);
    const std::vector<std::string> lines = split(std::string(bytes.begin(), bytes.end()), '\n');
    // the truth's contigs as ev::Targets, the hash made as dw_eval.cpp makes it
    const std::vector<std::string> head = split(lines.at(0), '\t');
    std::string names;
    std::vector<uint32_t> off(1, 0);
    for (size_t i = 1; i < head.size(); ++i) { names += head[i]; off.push_back((uint32_t)names.size()); }
    const int32_t nt = (int32_t)off.size() - 1;
    uint32_t hs = 2;
    while (hs < 2u * (uint32_t)nt) hs <<= 1;
    std::vector<int32_t> hash(hs, -1);
    for (int32_t t = 0; t < nt; ++t) {
        uint32_t h = ev::fnv1a(names.data() + off[t], off[t + 1] - off[t]) & (hs - 1);
        while (hash[h] >= 0) h = (h + 1) & (hs - 1);
        hash[h] = t;
    }
    const ev::Targets T = {names.data(), off.data(), hash.data(), nt, hs - 1};
    for (size_t li = 1; li < lines.size(); ++li) {
        if (lines[li].empty()) continue;
        const std::vector<std::string> part = split(lines[li], '|');
        if (part.size() != 3) { fprintf(stderr, "case %zu: three parts expected\n", li); return 2; }
        // heap copies of exactly the lines' bytes
        char *tl = (char *)malloc(part[0].size()), *al = (char *)malloc(part[1].size());
        memcpy(tl, part[0].data(), part[0].size());
        memcpy(al, part[1].data(), part[1].size());
        ev::TruthLine t;
        const int code = ev::truth_parse(tl, (uint32_t)part[0].size(), T, &t);
        if (code) { fprintf(stderr, "case %zu: truth line refused (%d)\n", li, code); return 1; }
        const uint32_t words = (t.unmapped || t.one_m) ? 0 : t.n_ops;
        uint32_t *pool = (uint32_t *)malloc(words ? words * sizeof(uint32_t) : 1);
        const ev::TruthRec rec = ev::truth_pack(tl, t, pool, 0);
        ev::Rec R;
        if (!ev::parse_sam_line(al, (uint32_t)part[1].size(), &R)) { fprintf(stderr, "case %zu: aligned line refused\n", li); return 1; }
        int contig = 0, n_ref = 0, used = 0;
        if (sscanf(part[2].c_str(), "%d %d %n", &contig, &n_ref, &used) < 2) { fprintf(stderr, "case %zu: bad third part\n", li); return 2; }
        ev::TruthCmp a, b;
        ev::truth_compare(R, contig, rec, pool, &a);
        const std::string hex = part[2].substr((size_t)used);
        uint8_t *bam = (uint8_t *)malloc(hex.size() / 2 + 1);
        for (size_t i = 0; i + 1 < hex.size(); i += 2) bam[i / 2] = (uint8_t)strtoul(hex.substr(i, 2).c_str(), nullptr, 16);
        ev::Rec B;
        if (!ev::parse_bam_record(bam, ev::ld32(bam), n_ref, &B)) { fprintf(stderr, "case %zu: BAM record refused\n", li); return 1; }
        ev::truth_compare(B, contig, rec, pool, &b);
        if (a.outcome != b.outcome || a.bases != b.bases || a.right != b.right || a.clipped != b.clipped || a.ibases != b.ibases || a.iright != b.iright ||
            a.exact != b.exact) {
            fprintf(stderr, "case %zu: the BAM front differs\n", li);
            return 1;
        }
        // the key of both records through either front
        uint64_t h1, h2, g1, g2;
        ev::key_hash(R.qname, (uint32_t)R.qlen, ev::key_end(R.flag), &h1, &h2);
        ev::key_hash(B.qname, (uint32_t)B.qlen, ev::key_end(B.flag), &g1, &g2);
        if (h1 != g1 || h2 != g2) { fprintf(stderr, "case %zu: the fronts hash the key differently\n", li); return 1; }
        print(a);
        free(bam); free(pool); free(tl); free(al);
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 4 && !strcmp(argv[1], "gz")) return run_gz(argv[2], argv[3]);
    if (argc == 3 && !strcmp(argv[1], "cmp")) return run_cmp(argv[2]);
    fprintf(stderr, "usage: eval_truth_main gz GZ PLAIN | cmp CASES\n");
    return 2;
}
