// dw_inflate.hpp -- a plain C++17 RFC 1951 inflater (stored, fixed and dynamic blocks) and a CRC-32, with no dependency: the host side of
// dwgsim_eval-hip's BAM input (dw_bam.hpp) inflates BGZF blocks with it on worker threads, so the library links no zlib.
//
// inflate() never reads past src + src_len and never writes past dst + dst_cap, whatever the input holds.  It rejects code sets that are
// over-subscribed or incomplete (a single code of length 1 is the one incomplete set zlib accepts, for literals and distances; so here), a
// missing end-of-block code, distances that reach in front of dst, the length symbols 286 / 287, the distance symbols 30 / 31, a stored block
// whose LEN and NLEN disagree and the reserved block type 3.
//
// Decoding: a 64-bit bit buffer, refilled eight bytes at a time away from the end of the input; one table of 2^11 entries per code set answers
// every code of up to 11 bits in one look-up, and the few longer ones are walked bit by bit over the canonical counts.
//
// gzip_member() reads one member of a gzip file over it (dwgsim_eval-hip -T: dwgsim-hip's truth SAM is a chain of members without size fields).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace dw {
namespace zz {

enum { Z_OK = 0, Z_E_TRUNCATED = -1, Z_E_BLOCK_TYPE = -2, Z_E_STORED = -3, Z_E_CODES = -4, Z_E_SYMBOL = -5, Z_E_DISTANCE = -6, Z_E_ROOM = -7 };

inline const char *error_name(int e)
{
    switch (e) {
    case Z_OK: return "ok";
    case Z_E_TRUNCATED: return "deflate stream ends early";
    case Z_E_BLOCK_TYPE: return "reserved deflate block type";
    case Z_E_STORED: return "stored block lengths disagree";
    case Z_E_CODES: return "invalid code lengths";
    case Z_E_SYMBOL: return "invalid code";
    case Z_E_DISTANCE: return "distance reaches in front of the output";
    default: return "more output than the block announces";
    }
}

constexpr int FAST_BITS = 11, MAX_BITS = 15;

// one canonical Huffman code set: fast[reversed code bits] = (symbol << 4) | length for lengths <= FAST_BITS, 0 otherwise
struct Huff {
    uint16_t fast[1 << FAST_BITS];
    uint16_t count[MAX_BITS + 1];
    uint16_t symbol[288];
};

// Z_OK, or Z_E_CODES for an over-subscribed set, or an incomplete one unless `one_ok` and it is a single code of length 1
inline int huff_build(Huff &h, const uint8_t *len, int n, bool one_ok)
{
    memset(h.fast, 0, sizeof h.fast);
    memset(h.count, 0, sizeof h.count);
    for (int s = 0; s < n; ++s) h.count[len[s]]++;
    int left = 1, used = n - h.count[0];
    for (int l = 1; l <= MAX_BITS; ++l) {
        left = (left << 1) - h.count[l];
        if (left < 0) return Z_E_CODES;
    }
    if (left > 0 && !(used == 0 || (one_ok && used == 1 && h.count[1] == 1))) return Z_E_CODES;
    uint16_t offs[MAX_BITS + 2], code[MAX_BITS + 2];
    offs[1] = 0; code[1] = 0;
    for (int l = 1; l <= MAX_BITS; ++l) {
        offs[l + 1] = (uint16_t)(offs[l] + h.count[l]);
        code[l + 1] = (uint16_t)((code[l] + h.count[l]) << 1);
    }
    for (int s = 0; s < n; ++s) {
        const int l = len[s];
        if (!l) continue;
        h.symbol[offs[l]++] = (uint16_t)s;
        const uint32_t c = code[l]++;
        if (l > FAST_BITS) continue;
        uint32_t r = 0;
        for (int b = 0; b < l; ++b) r |= ((c >> b) & 1u) << (l - 1 - b);
        for (uint32_t k = r; k < (1u << FAST_BITS); k += 1u << l) h.fast[k] = (uint16_t)((s << 4) | l);
    }
    h.count[0] = 0;
    return Z_OK;
}

struct Bits {
    const uint8_t *p, *end;
    uint64_t buf = 0;
    int n = 0;                  // valid bits in buf; the bits above them are zero or the stream's next bits
    void refill()
    {
        if (end - p >= 8) {
            uint64_t w;
            memcpy(&w, p, 8);
#if defined(__BYTE_ORDER__) && __BYTE_ORDER__ == __ORDER_BIG_ENDIAN__
            w = __builtin_bswap64(w);
#endif
            buf |= w << n;              // (bits above n are then the stream's next bits: the next refill ORs the same values in again)
            p += (63 - n) >> 3;
            n |= 56;
        } else {
            while (n <= 56 && p < end) { buf |= (uint64_t)*p++ << n; n += 8; }
        }
    }
    bool take(int k, uint32_t *v)       // k <= 32
    {
        if (n < k) { refill(); if (n < k) return false; }
        *v = (uint32_t)(buf & ((1ull << k) - 1));
        buf >>= k; n -= k;
        return true;
    }
};

// the next symbol of code set h, or a negative error
inline int huff_decode(Bits &b, const Huff &h)
{
    if (b.n < MAX_BITS) b.refill();
    const uint16_t e = h.fast[b.buf & ((1u << FAST_BITS) - 1)];
    if (e) {
        const int l = e & 15;
        if (l > b.n) return Z_E_TRUNCATED;
        b.buf >>= l; b.n -= l;
        return e >> 4;
    }
    int code = 0, first = 0, index = 0;
    for (int l = 1; l <= MAX_BITS; ++l) {
        code |= (int)((b.buf >> (l - 1)) & 1);
        const int cnt = h.count[l];
        if (code - cnt < first) {
            if (l > b.n) return Z_E_TRUNCATED;
            b.buf >>= l; b.n -= l;
            return h.symbol[index + (code - first)];
        }
        index += cnt; first += cnt;
        first <<= 1; code <<= 1;
    }
    return b.n < MAX_BITS ? Z_E_TRUNCATED : Z_E_SYMBOL;
}

// Inflates the raw deflate stream src[0, src_len) into dst[0, dst_cap): Z_OK and *dst_len, or a Z_E_* error (then *dst_len is what was
// written before it).  Bytes of src after the final block are ignored; *src_used says how many the stream took (the last one may be partly used),
// so that a caller can find what follows it: a gzip member's CRC-32 and ISIZE, and the next member.
inline int inflate_used(const uint8_t *src, size_t src_len, uint8_t *dst, size_t dst_cap, size_t *dst_len, size_t *src_used)
{
    static const uint16_t LEN_BASE[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    static const uint8_t LEN_EXTRA[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
    static const uint16_t DIST_BASE[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
    static const uint8_t DIST_EXTRA[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
    static const uint8_t CL_ORDER[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    Bits b;
    b.p = src; b.end = src + src_len;
    size_t out = 0;
    *dst_len = 0;
    Huff lit, dist;
    uint32_t last = 0;
    while (!last) {
        uint32_t type;
        if (!b.take(1, &last) || !b.take(2, &type)) return Z_E_TRUNCATED;
        if (type == 3) return Z_E_BLOCK_TYPE;
        if (type == 0) {
            // the rest of the byte is dropped; whole bytes already in the bit buffer go back to the input
            const int drop = b.n & 7;
            b.buf >>= drop; b.n -= drop;
            b.p -= b.n >> 3;
            b.buf = 0; b.n = 0;
            if (b.end - b.p < 4) return Z_E_TRUNCATED;
            const uint32_t len = b.p[0] | (uint32_t)b.p[1] << 8, nlen = b.p[2] | (uint32_t)b.p[3] << 8;
            b.p += 4;
            if ((len ^ nlen) != 0xFFFFu) return Z_E_STORED;
            if ((size_t)(b.end - b.p) < len) return Z_E_TRUNCATED;
            if (dst_cap - out < len) return Z_E_ROOM;
            if (len) memcpy(dst + out, b.p, len);
            out += len; b.p += len;
            *dst_len = out;
            continue;
        }
        uint8_t lens[320];
        if (type == 1) {
            for (int s = 0; s < 288; ++s) lens[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8;
            huff_build(lit, lens, 288, false);
            for (int s = 0; s < 32; ++s) lens[s] = 5;
            huff_build(dist, lens, 32, false);
        } else {
            uint32_t hlit, hdist, hclen;
            if (!b.take(5, &hlit) || !b.take(5, &hdist) || !b.take(4, &hclen)) return Z_E_TRUNCATED;
            hlit += 257; hdist += 1; hclen += 4;
            if (hlit > 286 || hdist > 30) return Z_E_CODES;
            uint8_t cl[19] = {0};
            for (uint32_t k = 0; k < hclen; ++k) {
                uint32_t v;
                if (!b.take(3, &v)) return Z_E_TRUNCATED;
                cl[CL_ORDER[k]] = (uint8_t)v;
            }
            if (huff_build(lit, cl, 19, false)) return Z_E_CODES;        // (lit holds the code-length code until the lengths are read)
            uint32_t k = 0;
            while (k < hlit + hdist) {
                const int s = huff_decode(b, lit);
                if (s < 0) return s;
                if (s < 16) { lens[k++] = (uint8_t)s; continue; }
                uint32_t rep, v = 0;
                if (s == 16) {
                    if (k == 0) return Z_E_CODES;
                    v = lens[k - 1];
                    if (!b.take(2, &rep)) return Z_E_TRUNCATED;
                    rep += 3;
                } else if (s == 17) {
                    if (!b.take(3, &rep)) return Z_E_TRUNCATED;
                    rep += 3;
                } else {
                    if (!b.take(7, &rep)) return Z_E_TRUNCATED;
                    rep += 11;
                }
                if (k + rep > hlit + hdist) return Z_E_CODES;
                while (rep--) lens[k++] = (uint8_t)v;
            }
            if (lens[256] == 0) return Z_E_CODES;
            uint8_t dl[32];
            memcpy(dl, lens + hlit, hdist);
            if (huff_build(lit, lens, (int)hlit, true) || huff_build(dist, dl, (int)hdist, true)) return Z_E_CODES;
        }
        for (;;) {
            int s = huff_decode(b, lit);
            if (s < 0) return s;
            if (s < 256) {
                if (out == dst_cap) return Z_E_ROOM;
                dst[out++] = (uint8_t)s;
                continue;
            }
            if (s == 256) break;
            s -= 257;
            if (s >= 29) return Z_E_SYMBOL;
            uint32_t ex;
            if (!b.take(LEN_EXTRA[s], &ex)) return Z_E_TRUNCATED;
            const size_t len = LEN_BASE[s] + ex;
            const int d = huff_decode(b, dist);
            if (d < 0) return d;
            if (d >= 30) return Z_E_SYMBOL;
            if (!b.take(DIST_EXTRA[d], &ex)) return Z_E_TRUNCATED;
            const size_t back = DIST_BASE[d] + ex;
            if (back > out) return Z_E_DISTANCE;
            if (dst_cap - out < len) return Z_E_ROOM;
            const uint8_t *from = dst + out - back;
            uint8_t *to = dst + out;
            if (back >= len) memcpy(to, from, len);
            else for (size_t i = 0; i < len; ++i) to[i] = from[i];
            out += len;
        }
        *dst_len = out;
    }
    *dst_len = out;
    *src_used = (size_t)(b.p - src) - (size_t)(b.n >> 3);       // (whole bytes still in the bit buffer were not taken)
    return Z_OK;
}

inline int inflate(const uint8_t *src, size_t src_len, uint8_t *dst, size_t dst_cap, size_t *dst_len)
{
    size_t used;
    return inflate_used(src, src_len, dst, dst_cap, dst_len, &used);
}

// CRC-32 (IEEE 802.3, the gzip one), slicing-by-8
struct CrcTable {
    uint32_t t[8][256];
    CrcTable()
    {
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1)));
            t[0][i] = c;
        }
        for (uint32_t i = 0; i < 256; ++i)
            for (int k = 1; k < 8; ++k) t[k][i] = (t[k - 1][i] >> 8) ^ t[0][t[k - 1][i] & 0xff];
    }
};

inline uint32_t crc32(const uint8_t *p, size_t n, uint32_t crc = 0)
{
    static const CrcTable T;
    uint32_t c = ~crc;
    while (n >= 8) {
        const uint32_t a = c ^ ((uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24);
        c = T.t[7][a & 0xff] ^ T.t[6][(a >> 8) & 0xff] ^ T.t[5][(a >> 16) & 0xff] ^ T.t[4][a >> 24] ^ T.t[3][p[4]] ^ T.t[2][p[5]] ^ T.t[1][p[6]] ^ T.t[0][p[7]];
        p += 8; n -= 8;
    }
    while (n--) c = (c >> 8) ^ T.t[0][(c ^ *p++) & 0xff];
    return ~c;
}

// One member of a gzip file (RFC 1952) at src[0, src_len): its deflate stream is data_off bytes in.  false and *why for a header that is not
// gzip's, uses another method than deflate, or does not fit in the bytes.
inline bool gzip_member_header(const uint8_t *src, size_t src_len, size_t *data_off, const char **why)
{
    *why = "the gzip member header is cut short";
    if (src_len < 10) return false;
    if (src[0] != 0x1f || src[1] != 0x8b) { *why = "not a gzip member"; return false; }
    if (src[2] != 8 || (src[3] & 0xe0)) { *why = "unknown gzip method or flags"; return false; }
    const uint8_t flg = src[3];
    size_t p = 10;
    if (flg & 4) {              // FEXTRA
        if (src_len - p < 2) return false;
        const size_t xlen = src[p] | (size_t)src[p + 1] << 8;
        p += 2;
        if (src_len - p < xlen) return false;
        p += xlen;
    }
    for (int bit = 8; bit <= 16; bit <<= 1)         // FNAME, FCOMMENT: zero-terminated
        if (flg & bit) {
            while (p < src_len && src[p]) ++p;
            if (p == src_len) return false;
            ++p;
        }
    if (flg & 2) {              // FHCRC
        if (src_len - p < 2) return false;
        p += 2;
    }
    *data_off = p;
    return true;
}

// Inflates the member at src into dst[0, dst_cap): Z_OK, *dst_len and *member_len (header, stream and the eight bytes behind it), after the
// member's CRC-32 and ISIZE were checked; Z_E_ROOM asks for a larger dst; any other failure is < 0 with *why.
inline int gzip_member(const uint8_t *src, size_t src_len, uint8_t *dst, size_t dst_cap, size_t *dst_len, size_t *member_len, const char **why)
{
    size_t off;
    *dst_len = 0;
    if (!gzip_member_header(src, src_len, &off, why)) return Z_E_TRUNCATED;
    size_t used = 0;
    const int r = inflate_used(src + off, src_len - off, dst, dst_cap, dst_len, &used);
    *why = error_name(r);
    if (r) return r;
    if (src_len - off - used < 8) { *why = "the gzip member ends before its CRC-32 and ISIZE"; return Z_E_TRUNCATED; }
    const uint8_t *t = src + off + used;
    const uint32_t crc = t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
    const uint32_t isize = t[4] | (uint32_t)t[5] << 8 | (uint32_t)t[6] << 16 | (uint32_t)t[7] << 24;
    if (isize != (uint32_t)*dst_len) { *why = "ISIZE differs from the inflated size"; return Z_E_SYMBOL; }
    if (crc != crc32(dst, *dst_len)) { *why = "CRC-32 mismatch"; return Z_E_SYMBOL; }
    *member_len = off + used + 8;
    return Z_OK;
}

} // namespace zz
} // namespace dw
