// dw_bam.hpp -- the host side of BAM input for dwgsim_eval-hip (dw_eval.cpp): BGZF framing, the inflate seam and its worker threads, the BAM
// header, and BAM record -> SAM text for -p and the fatal-record messages.  Plain C++17, no HIP and no zlib (dw_inflate.hpp does the work).
//
// BGZF (SAM spec 4.1): a file is a series of gzip members of at most 64 KiB each, whose extra field holds a subfield `BC` with the member's
// total size minus one; the member ends in CRC-32 and ISIZE of its data.  bgzf_block_at() frames one; the 28-byte end-of-file marker is an
// ordinary block with no data, and so is any other empty block.  A file may end at a block boundary without the marker.
//
// The seam: inflate_blocks() is the one place where compressed bytes become data.  It takes jobs whose destinations were fixed beforehand from
// the ISIZE fields, so every block is independent; here a pool of host threads runs dw::zz::inflate and checks ISIZE and CRC-32 on each.
// A device inflater would replace this function and nothing else.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <atomic>
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include "dw_inflate.hpp"

namespace dw {
namespace bam {

inline uint32_t le16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
inline uint32_t le32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

constexpr uint32_t BGZF_MAX_ISIZE = 65536;

struct BgzfBlock {
    size_t size;            // of the whole member
    size_t data_off, data_len;      // the deflate stream inside it
    uint32_t crc, isize;
};

// The block that starts at p, of which `avail` bytes are there: 1 and *b; 0 when more bytes are needed to tell; -1 and *why when it is none.
inline int bgzf_block_at(const uint8_t *p, size_t avail, BgzfBlock *b, const char **why)
{
    if (avail >= 1 && p[0] != 0x1f) { *why = "not a gzip (BGZF) file"; return -1; }
    if (avail >= 2 && p[1] != 0x8b) { *why = "not a gzip (BGZF) file"; return -1; }
    if (avail < 12) return 0;
    if (p[2] != 8 || !(p[3] & 4) || (p[3] & 0x1a)) { *why = "a gzip member without the BGZF extra field"; return -1; }
    const size_t xlen = le16(p + 10);
    if (avail < 12 + xlen) return 0;
    size_t bsize = 0;
    for (size_t q = 12; q + 4 <= 12 + xlen;) {
        const size_t slen = le16(p + q + 2);
        if (q + 4 + slen > 12 + xlen) break;
        if (p[q] == 'B' && p[q + 1] == 'C' && slen == 2) { bsize = (size_t)le16(p + q + 4) + 1; break; }
        q += 4 + slen;
    }
    if (!bsize) { *why = "a gzip member without the BGZF BC subfield"; return -1; }
    if (bsize < 12 + xlen + 8) { *why = "a BGZF block smaller than its own header"; return -1; }
    if (avail < bsize) return 0;
    b->size = bsize;
    b->data_off = 12 + xlen;
    b->data_len = bsize - 8 - b->data_off;
    b->crc = le32(p + bsize - 8);
    b->isize = le32(p + bsize - 4);
    if (b->isize > BGZF_MAX_ISIZE) { *why = "a BGZF block that announces more than 64 KiB"; return -1; }
    return 1;
}

// one block for the inflater: src[0, src_len) inflates to exactly isize bytes at dst, whose CRC-32 is crc.  error: nullptr when all held.
struct InflateJob {
    const uint8_t *src;
    size_t src_len;
    uint8_t *dst;
    uint32_t isize, crc;
    const char *error;
};

inline void inflate_job(InflateJob &j)
{
    size_t got = 0;
    const int r = zz::inflate(j.src, j.src_len, j.dst, j.isize, &got);
    j.error = r ? zz::error_name(r) : got != j.isize ? "ISIZE differs from the inflated size" : zz::crc32(j.dst, got) != j.crc ? "CRC-32 mismatch" : nullptr;
}

// `threads` - 1 workers plus the calling thread, which share the jobs of one inflate_blocks() call through a counter
class InflatePool {
public:
    explicit InflatePool(int threads)
    {
        for (int i = 1; i < threads; ++i) th_.emplace_back([this] { worker(); });
    }
    ~InflatePool()
    {
        {
            std::lock_guard<std::mutex> l(m_);
            quit_ = true;
        }
        cv_.notify_all();
        for (auto &t : th_) t.join();
    }
    InflatePool(const InflatePool &) = delete;
    InflatePool &operator=(const InflatePool &) = delete;

    void run(InflateJob *jobs, size_t n)
    {
        if (th_.empty() || n < 2) {
            for (size_t i = 0; i < n; ++i) inflate_job(jobs[i]);
            return;
        }
        {
            std::lock_guard<std::mutex> l(m_);
            jobs_ = jobs; n_ = n; next_.store(0); active_ = (int)th_.size(); ++gen_;
        }
        cv_.notify_all();
        work();
        std::unique_lock<std::mutex> l(m_);
        done_.wait(l, [this] { return active_ == 0; });
    }

private:
    void work()
    {
        for (size_t i; (i = next_.fetch_add(1)) < n_;) inflate_job(jobs_[i]);
    }
    void worker()
    {
        uint64_t seen = 0;
        for (;;) {
            {
                std::unique_lock<std::mutex> l(m_);
                cv_.wait(l, [&] { return quit_ || gen_ != seen; });
                if (quit_) return;
                seen = gen_;
            }
            work();
            std::lock_guard<std::mutex> l(m_);
            if (--active_ == 0) done_.notify_one();
        }
    }
    std::vector<std::thread> th_;
    std::mutex m_;
    std::condition_variable cv_, done_;
    InflateJob *jobs_ = nullptr;
    size_t n_ = 0;
    std::atomic<size_t> next_{0};
    uint64_t gen_ = 0;
    int active_ = 0;
    bool quit_ = false;
};

// THE SEAM: all jobs done (each job's error set) when it returns
inline void inflate_blocks(InflatePool &pool, InflateJob *jobs, size_t n) { pool.run(jobs, n); }

// ---- BAM header: magic, l_text, text, n_ref, then l_name, name, l_ref per reference ----
struct Header {
    std::string text;               // l_text bytes, cut at a NUL
    std::string names;              // the reference names, concatenated
    std::vector<uint32_t> off;      // names[off[t], off[t+1])
};

// the header at the start of d[0, n): its size in bytes (> 0) and *h; 0 when d ends inside it; -1 and *why when it is none
inline int64_t parse_header(const uint8_t *d, size_t n, Header *h, const char **why)
{
    for (size_t k = 0; k < 4 && k < n; ++k)
        if (d[k] != (uint8_t)"BAM\1"[k]) { *why = "bad BAM magic"; return -1; }
    if (n < 8) return 0;
    const int32_t l_text = (int32_t)le32(d + 4);
    if (l_text < 0) { *why = "negative l_text in the BAM header"; return -1; }
    size_t p = 8 + (size_t)l_text;
    if (n < p + 4) return 0;
    const int32_t n_ref = (int32_t)le32(d + p);
    if (n_ref < 0) { *why = "negative n_ref in the BAM header"; return -1; }
    p += 4;
    h->names.clear();
    h->off.assign(1, 0);
    for (int32_t t = 0; t < n_ref; ++t) {
        if (n < p + 4) return 0;
        const int32_t l_name = (int32_t)le32(d + p);
        if (l_name < 1) { *why = "a reference name length below 1 in the BAM header"; return -1; }
        p += 4;
        if (n < p + (size_t)l_name + 4) return 0;
        h->names.append((const char *)d + p, strnlen((const char *)d + p, (size_t)l_name));
        h->off.push_back((uint32_t)h->names.size());
        p += (size_t)l_name + 4;
    }
    h->text.assign((const char *)d + 8, strnlen((const char *)d + 8, (size_t)l_text));
    return (int64_t)p;
}

// ---- a BAM record that parse_bam_record accepted, as a SAM line (no newline) ----
inline void append_int(std::string &s, long long v)
{
    char b[32];
    snprintf(b, sizeof b, "%lld", v);
    s += b;
}

inline void append_float(std::string &s, const uint8_t *p)
{
    float f;
    const uint32_t w = le32(p);
    memcpy(&f, &w, 4);
    char b[64];
    snprintf(b, sizeof b, "%g", (double)f);
    s += b;
}

// a typed number of an aux field (types c C s S i I f): its size, 0 for another type
inline size_t aux_number(std::string *s, uint8_t ty, const uint8_t *p, size_t room)
{
    const size_t size = (ty == 'c' || ty == 'C') ? 1 : (ty == 's' || ty == 'S') ? 2 : (ty == 'i' || ty == 'I' || ty == 'f') ? 4 : 0;
    if (!size || room < size || !s) return room < size ? 0 : size;
    switch (ty) {
    case 'c': append_int(*s, (int8_t)p[0]); break;
    case 'C': append_int(*s, p[0]); break;
    case 's': append_int(*s, (int16_t)le16(p)); break;
    case 'S': append_int(*s, le16(p)); break;
    case 'i': append_int(*s, (int32_t)le32(p)); break;
    case 'I': append_int(*s, le32(p)); break;
    default: append_float(*s, p); break;
    }
    return size;
}

inline void record_to_sam(const uint8_t *rec, const Header &h, std::string &s)
{
    const uint32_t block_size = le32(rec);
    const uint8_t *f = rec + 4, *end = rec + 4 + block_size;
    const int32_t ref_id = (int32_t)le32(f), pos = (int32_t)le32(f + 4), l_seq = (int32_t)le32(f + 16), next_ref = (int32_t)le32(f + 20),
                  next_pos = (int32_t)le32(f + 24), tlen = (int32_t)le32(f + 28);
    const uint32_t l_name = f[8], mapq = f[9], n_cigar = le16(f + 12), flag = le16(f + 14);
    const int32_t n_ref = (int32_t)h.off.size() - 1;
    auto ref_name = [&](int32_t t) {
        if (t < 0 || t >= n_ref) s += '*';
        else s.append(h.names, h.off[t], h.off[t + 1] - h.off[t]);
    };
    const uint8_t *name = f + 32;
    s.append((const char *)name, strnlen((const char *)name, l_name));
    s += '\t'; append_int(s, flag);
    s += '\t'; ref_name(ref_id);
    s += '\t'; append_int(s, (long long)pos + 1);
    s += '\t'; append_int(s, mapq);
    s += '\t';
    const uint8_t *cg = name + l_name;
    if (!n_cigar) s += '*';
    for (uint32_t k = 0; k < n_cigar; ++k) {
        const uint32_t w = le32(cg + 4 * k);
        append_int(s, w >> 4);
        s += (w & 15) < 9 ? "MIDNSHP=X"[w & 15] : '?';
    }
    s += '\t';
    if (next_ref < 0) s += '*';
    else if (next_ref == ref_id) s += '=';
    else ref_name(next_ref);
    s += '\t'; append_int(s, (long long)next_pos + 1);
    s += '\t'; append_int(s, tlen);
    s += '\t';
    const uint8_t *seq = cg + 4 * (size_t)n_cigar, *qual = seq + ((size_t)l_seq + 1) / 2;
    if (!l_seq) s += '*';
    for (int32_t k = 0; k < l_seq; ++k) s += "=ACMGRSVTWYHKDBN"[(seq[k >> 1] >> ((k & 1) ? 0 : 4)) & 15];
    s += '\t';
    if (!l_seq || qual[0] == 0xff) s += '*';
    else for (int32_t k = 0; k < l_seq; ++k) s += (char)(qual[k] + 33);
    // aux fields, up to the first one that cannot be read whole
    for (const uint8_t *p = qual + l_seq; end - p >= 3;) {
        const uint8_t ty = p[2];
        const uint8_t *v = p + 3;
        std::string t = "\t";
        t += (char)p[0]; t += (char)p[1]; t += ':';
        if (ty == 'A') {
            if (end - v < 1) break;
            t += "A:"; t += (char)v[0];
            p = v + 1;
        } else if (ty == 'Z' || ty == 'H') {
            const uint8_t *q = v;
            while (q < end && *q) ++q;
            if (q == end) break;
            t += (char)ty; t += ':';
            t.append((const char *)v, q - v);
            p = q + 1;
        } else if (ty == 'B') {
            if (end - v < 5) break;
            const uint8_t st = v[0];
            const uint64_t cnt = le32(v + 1), es = aux_number(nullptr, st, v + 5, 8);
            if (!es || (uint64_t)(end - (v + 5)) < es * cnt) break;
            t += "B:"; t += (char)st;
            for (uint64_t k = 0; k < cnt; ++k) { t += ','; aux_number(&t, st, v + 5 + es * k, es); }
            p = v + 5 + es * cnt;
        } else {
            std::string num;
            const size_t size = aux_number(&num, ty, v, (size_t)(end - v));
            if (!size) break;
            t += ty == 'f' ? "f:" : "i:";
            t += num;
            p = v + size;
        }
        s += t;
    }
}

} // namespace bam
} // namespace dw
