// dw_truth.hpp -- the truth step: every simulated read end's true alignment as one SAM line (DESIGN.md "6e").  Included by dw_simulate.hip (DW_PART 0).
// Nothing of k_simulate is instrumented: the step runs behind it on the same stream and REPLAYS what it needs --
//   the accepted attempt and the random-read verdict of a pair from meta[pair] (the record k_simulate leaves for the abort rule),
//   placement, haplotype and strands from draw_pair / read_geom (dw_read.hpp: pure functions of seed, contig, read index and attempt),
//   the alignment from the haplotype's byte cells, by the per-cell law of gen_read (dw_read.hpp, "an episode of the reference's per-cell logic"),
//   QNAME, SEQ and QUAL from the finished FASTQ text (the name holds n_err, which only the error phase knows).
// Steps, the shape of k_hap_len -> k_scan_excl -> k_hap_write (dw_walk.hip):
//   k_truth_nl_count -> k_scan_excl -> k_truth_nl_index   where every FASTQ record of a source stream starts: every fourth newline ends one
//   k_truth_len, k_truth_len2                               one lane per read end: the replay and the travel walk; then, with the mate's record in reach, the bytes of its line
//   k_scan_excl                                            over the blocks' bytes: with the scan k_truth_len2 makes inside each block, where each line starts
//   k_truth_write                                           one lane per read end: the line, its CIGAR from a second walk over the cells (no CIGAR is ever stored)
// With dwgsim_hip_set_truth_depth (DESIGN.md "6f") k_truth_depth runs behind k_truth_len: the read ends it left, joined with the group's list of mutated cells
// into two counters per cell (the rule: at the kernel).  Without the truth SAM the step is k_truth_len<false, false> and k_truth_depth alone (launch_truth_depth).
// With dwgsim_hip_set_truth_md the three kernels run as their <true> instances (the <false> ones are the step as it was, to the instruction): the length pass also
// takes NM and the characters of MD (truth_tags), the sums are taken in 64 bits (k_truth_scan), the write pass spells MD out with a second truth_tags walk.
//
// The alignment of a read end.  gen_read starts at the first cell in travel order that is unmutated or substituted and stops once s bases have been
// produced; a deleted cell produces nothing, a cell with an insertion its own base and the inserted bases -- a forward read the base first, a reverse
// read (travelling down) the inserted bases first, last one first.  In reference order that is the cells lo .. hi, both of them cells that gave a
// base of their own (M), and
//   lead   inserted bases in front of lo's base: a reverse read that stopped inside (or at the end of) the insertion of a cell left of lo.  That
//          cell's own base is not part of the read, and deleted cells between it and lo are not part of the alignment: the line starts nI and POS is lo
//   tail   inserted bases behind hi's base, of hi's own insertion: a forward read that stopped inside (or at the end of) it
// so a CIGAR never starts or ends with D, always holds an M, and starts or ends with I exactly where the read stopped inside an insertion.
#pragma once
#include "dw_read.hpp"
#include "dw_launch.hpp"

namespace dw {

constexpr int TRUTH_NL_THREADS = 256, TRUTH_NL_BYTES = 16 * TRUTH_NL_THREADS;      // the record index: 16 bytes per lane, 4096 per block

// the newlines among the (at most sixteen) bytes of `text` at offset b that lie below n, as a bit mask
DW_DEV uint32_t truth_nl_mask(const uint8_t *text, uint64_t b, uint64_t n)
{
    if (b >= n) return 0;
    const uint4 q = *reinterpret_cast<const uint4 *>(text + b);      // (16-byte aligned; the buffer is padded behind its capacity)
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) if (((w[k >> 2] >> (8 * (k & 3))) & 0xffu) == (uint32_t)'\n') m |= 1u << k;
    const uint64_t left = n - b;
    return left < 16 ? m & ((1u << (uint32_t)left) - 1u) : m;
}
// newlines per block of TRUTH_NL_BYTES bytes of a text whose length is still on the device
__global__ void __launch_bounds__(TRUTH_NL_THREADS) k_truth_nl_count(const uint8_t *__restrict__ text, const uint64_t *__restrict__ n_dev, uint32_t *__restrict__ block_count)
{
    __shared__ uint32_t sm[17];
    const uint64_t b = ((uint64_t)blockIdx.x * TRUTH_NL_THREADS + threadIdx.x) * 16;
    uint32_t total;
    block_excl_scan((uint32_t)__popc(truth_nl_mask(text, b, *n_dev)), sm, &total);
    if (threadIdx.x == 0) block_count[blockIdx.x] = total;
}
// ... and, from their scan: rec[r] = where record r starts = behind newline 4 r - 1; rec[n_rec] = the end of the last one
__global__ void __launch_bounds__(TRUTH_NL_THREADS) k_truth_nl_index(const uint8_t *__restrict__ text, const uint64_t *__restrict__ n_dev, const uint32_t *__restrict__ block_base, uint32_t *__restrict__ rec, uint64_t n_rec)
{
    __shared__ uint32_t sm[17];
    const uint64_t b = ((uint64_t)blockIdx.x * TRUTH_NL_THREADS + threadIdx.x) * 16;
    uint32_t m = truth_nl_mask(text, b, *n_dev), total;
    uint32_t g = block_base[blockIdx.x] + block_excl_scan((uint32_t)__popc(m), sm, &total);      // newlines in front of this lane's bytes
    if (blockIdx.x == 0 && threadIdx.x == 0) rec[0] = 0;
    while (m) {
        const int k = __ffs((int)m) - 1; m &= m - 1; ++g;
        if ((g & 3u) == 0u && (uint64_t)(g >> 2) <= n_rec) rec[g >> 2] = (uint32_t)(b + (uint64_t)k + 1);
    }
}

// the insertion a cell stands for (0: the cell has no table entry and gives its own base alone)
DW_DEV uint32_t truth_ins_len(const HapDev &h, int32_t i)
{
    const uint32_t idx = ins_find(h, i);
    return idx < h.n_ins && (int64_t)h.ins_pos[idx] == (int64_t)i + h.pos_off ? h.ins_len[idx] : 0u;
}
// The travel walk: gen_read's per-cell law without the bases.  false: the walk left the contig (the attempt in meta was not an accepted one -- a batch
// that ends in an error -- and the line is not written).
DW_DEV bool truth_travel(const HapDev &h, int32_t l, int64_t start, int step, int s, TruthEnd &t)
{
    t.lo = t.hi = 0; t.lead = t.tail = 0;
    if (start < 0 || start >= (int64_t)l) return false;
    int32_t i = (int32_t)start, first = -1, last_m = -1; int k = 0;
    while (k < s) {
        if (i < 0 || i >= l) return false;
        // sixteen cells in one load where the read takes all of them and none is an INSERT or DELETE cell (h.cells is 16-byte aligned: dw_read.hpp, episodes): a
        // load per cell was a memory round trip per base
        if (s - k >= 16 && (step > 0 ? ((i & 15) == 0 && i + 16 <= l) : (i & 15) == 15)) {
            const uint4 q = *reinterpret_cast<const uint4 *>(h.cells + (step > 0 ? i : i - 15));
            if (((q.x | q.y | q.z | q.w) & 0x10101010u) == 0) { if (first < 0) first = i; k += 16; i += 16 * step; last_m = i - step; continue; }
        }
        const uint32_t mt = h.cells[i] & TMASK;
        if (first < 0) {
            if (mt != T_NONE && mt != T_SUB) { i += step; continue; }
            first = i;
        }
        if (mt == T_DEL) {}
        else if (mt != T_INS) { ++k; last_m = i; }
        else {
            const uint32_t n = truth_ins_len(h, i);
            if (step > 0) { ++k; last_m = i; const uint32_t take = n < (uint32_t)(s - k) ? n : (uint32_t)(s - k); k += (int)take; if (k >= s) t.tail = take; }
            else { const uint32_t take = n < (uint32_t)(s - k) ? n : (uint32_t)(s - k); k += (int)take; if (k < s) { ++k; last_m = i; } else t.lead = take; }
        }
        i += step;
    }
    if (step > 0) { t.lo = first; t.hi = last_m; } else { t.lo = last_m; t.hi = first; }
    return true;
}
// The CIGAR in reference order from (lo, hi, lead, tail): op(count, letter) for every run of equal operations
template <class F>
DW_DEV void truth_cigar(const HapDev &h, const TruthEnd &t, F &&op)
{
    uint32_t run = 0, cur = 0;
    auto add = [&](uint32_t n, uint32_t letter) {
        if (n == 0) return;
        if (letter == cur) { run += n; return; }
        if (run) op(run, cur);
        cur = letter; run = n;
    };
    add(t.lead, 'I');
    int32_t c = t.lo;
    while (c <= t.hi) {
        if ((c & 15) == 0 && c + 15 <= t.hi) {     // sixteen cells at once, as the travel walk takes them
            const uint4 q = *reinterpret_cast<const uint4 *>(h.cells + c);
            if (((q.x | q.y | q.z | q.w) & 0x10101010u) == 0) { add(16, 'M'); c += 16; continue; }
        }
        if ((c & 3) == 0 && c + 3 <= t.hi) {      // four cells at once: nothing mutated but by substitution among them (h.cells is 16-byte aligned)
            const uint32_t w = *reinterpret_cast<const uint32_t *>(h.cells + c);
            if (((w & 0x10101010u) == 0)) { add(4, 'M'); c += 4; continue; }
        }
        const uint32_t mt = h.cells[c] & TMASK;
        if (mt == T_DEL) add(1, 'D');
        else { add(1, 'M'); if (mt == T_INS) add(c == t.hi ? t.tail : truth_ins_len(h, c), 'I'); }
        ++c;
    }
    if (run) op(run, cur);
}
template <class O, int N>
DW_DEV void truth_lit(O &o, const char (&s)[N]) { for (int i = 0; i < N - 1; ++i) o.put((uint32_t)(uint8_t)s[i]); }
DW_DEV uint32_t truth_ndigits(uint32_t v) { uint32_t n = 1; while (v >= 10u) { v /= 10u; ++n; } return n; }
template <class O>
DW_DEV void truth_put_dec(O &o, uint32_t v)
{
    uint32_t p = 1; while (v / p >= 10u) p *= 10u;
    for (; p; p /= 10u) o.put((uint32_t)'0' + (v / p) % 10u);
}

// ---- NM:i: and MD:Z: (dwgsim_hip_set_truth_md) ----
// The law (samtools calmd's convention, restated).  Walk the CIGAR in reference order from POS.  r = the reference letter of a cell: A C G T for the codes
// 0-3, N for every other code, always upper case.  b = the base of SEQ as the line prints it (reverse-complemented under 0x10); a leading I run takes the
// first `lead` bases of SEQ.
//   M cell     a match if and only if b == r and r is one of ACGT (N against N is a mismatch).  A match adds one to the running count; a mismatch emits the
//              count, then r, sets the count to 0 and adds 1 to NM
//   I run, n   NM += n; MD is not touched and the count runs on
//   D run, n   the count, '^', the n reference letters; the count is 0 again; NM += n
//   the end    the count, also when it is 0
// so MD matches [0-9]+(([A-Z]|\^[A-Z]+)[0-9]+)* and a mismatch directly behind a deletion gets its 0 (^AC0T).
// Nothing of it is instrumented: SEQ (the finished FASTQ text, errors included) against the reference codes along the replayed alignment is the answer.
DW_DEV uint32_t truth_ref_letter(uint32_t code) { return code < 4u ? (0x54474341u >> (8u * code)) & 0xffu : (uint32_t)'N'; }
// eight base codes 0 .. 3, one per byte, as their letters: 'A' + 2 (bit 0) + 6 (bit 1) + 11 (both)
DW_DEV uint64_t truth_letters8(uint64_t c)
{
    const uint64_t one = 0x0101010101010101ull, b0 = c & one, b1 = (c >> 1) & one;
    return 0x41ull * one + 2ull * b0 + 6ull * b1 + 11ull * (b0 & b1);
}
DW_DEV uint32_t truth_comp(uint32_t b) { return b == 'A' ? (uint32_t)'T' : b == 'T' ? (uint32_t)'A' : b == 'C' ? (uint32_t)'G' : b == 'G' ? (uint32_t)'C' : b; }
// The walk of the tags: the cells lo .. hi in reference order with the reference and the read beside them.  ref: the codes of the contig (its cell 0); seq: the s
// bases of the FASTQ record; rev: the line prints them reverse-complemented.  num(n): a count of the MD string, ch(c): one character of it.  Returns NM.
// Sixteen cells per step from wherever the walk stands -- the record's bases lie at the record's own phase anyway, and gfx950 takes 16-byte loads at any address
// -- of which the ones in front of the first INSERT or DELETE cell (and inside lo .. hi) count: their reference codes as letters (a reverse read: of the
// complement) against as many bases of the record as they stand.  The common case is sixteen matches that only add to the count; a cell that differs, or holds no
// ACGT, is taken out of the difference one at a time.  The INSERT or DELETE cell that ended the step is taken singly, a run of DELETE cells out of the same load.
// (The loads run up to fifteen bytes past what counts: cells and reference codes are padded by CELL_PAD behind the group, the text buffers by 64 bytes; a reverse
// read's last step reads in front of its bases, into its own name line: the caller vouches for TRUTH_MD_QNAME_MIN characters of QNAME -- a read name has 26 at least.)
constexpr uint32_t TRUTH_MD_QNAME_MIN = 14;      // '@' + QNAME + '\n' in front of the bases: sixteen bytes at least (a record that has fewer gets no line: k_truth_len<true>)
template <class N, class C>
DW_DEV uint32_t truth_tags(const HapDev &h, const uint8_t *ref, const TruthEnd &t, const uint8_t *seq, uint32_t s, bool rev, N &&num, C &&ch)
{
    uint32_t nm = t.lead, q = t.lead, run = 0; bool del = false;
    const uint64_t turn = rev ? 0x0303030303030303ull : 0ull, other = 0xfcfcfcfcfcfcfcfcull;
    auto byte_of = [](uint64_t lo, uint64_t hi, uint32_t k) -> uint32_t { return (uint32_t)((k < 8u ? lo : hi) >> (8u * (k & 7u))) & 0xffu; };
    auto m_cell = [&](uint32_t code) {      // one M cell against the next base of SEQ
        const uint32_t b = rev ? truth_comp(seq[s - 1u - q]) : (uint32_t)seq[q];
        ++q; del = false;
        const bool same = code < 4u && b == truth_ref_letter(code);
        if (!same) { num(run); ch(truth_ref_letter(code)); }
        run = same ? run + 1u : 0u; nm += same ? 0u : 1u;      // (as selects: an increment of either one behind a branch was merged into one through memory)
    };
    int32_t c = t.lo;
    while (c <= t.hi) {
        const uint32_t left = (uint32_t)(t.hi - c) + 1u, lim = left < 16u ? left : 16u;
        const uint64_t m0 = reinterpret_cast<const Unal16 *>(h.cells + c)->a, m1 = reinterpret_cast<const Unal16 *>(h.cells + c)->b;
        const uint64_t r0 = reinterpret_cast<const Unal16 *>(ref + c)->a, r1 = reinterpret_cast<const Unal16 *>(ref + c)->b;
        const uint64_t i0 = m0 & 0x1010101010101010ull, i1 = m1 & 0x1010101010101010ull;
        uint32_t n = i0 ? (uint32_t)__builtin_ctzll(i0) >> 3 : i1 ? 8u + ((uint32_t)__builtin_ctzll(i1) >> 3) : 16u;      // cells in front of the first INSERT / DELETE cell
        if (n > lim) n = lim;
        if (n) {
            uint64_t e0, e1;      // the bases at positions q .. q + 15 of the printed SEQ, uncomplemented
            if (rev) { const uint8_t *p = seq + (s - q); e0 = __builtin_bswap64(reinterpret_cast<const Unal8 *>(p - 8)->v); e1 = __builtin_bswap64(reinterpret_cast<const Unal8 *>(p - 16)->v); }
            else { e0 = reinterpret_cast<const Unal16 *>(seq + q)->a; e1 = reinterpret_cast<const Unal16 *>(seq + q)->b; }
            uint64_t d0 = (truth_letters8((r0 ^ turn) & ~other) ^ e0) | (r0 & other), d1 = (truth_letters8((r1 ^ turn) & ~other) ^ e1) | (r1 & other);
            if (n < 8u) { d0 &= (1ull << (8u * n)) - 1ull; d1 = 0; }
            else if (n < 16u) d1 &= (1ull << (8u * (n - 8u))) - 1ull;      // (n = 8: nothing of d1)
            if ((d0 | d1) == 0) run += n;
            else {
                uint32_t prev = 0;
                auto differ = [&](uint64_t d, uint64_t r, uint32_t first) {      // the cells of one half that differ, in order
                    while (d) {
                        const uint32_t k = (uint32_t)__builtin_ctzll(d) >> 3, at = first + k;
                        d &= ~(0xffull << (8u * k));
                        num(run + (at - prev)); ch(truth_ref_letter((uint32_t)(r >> (8u * k)) & 0xffu)); run = 0; prev = at + 1u; ++nm;
                    }
                };
                differ(d0, r0, 0u); differ(d1, r1, 8u);
                run += n - prev;
            }
            q += n; c += (int32_t)n; del = false;
        }
        if (n == lim) continue;      // no INSERT or DELETE cell among them
        if ((byte_of(m0, m1, n) & TMASK) == T_DEL) {
            if (!del) { num(run); ch('^'); run = 0; del = true; }
            for (uint32_t k = n; k < lim && (byte_of(m0, m1, k) & TMASK) == T_DEL; ++k, ++c) { ch(truth_ref_letter(byte_of(r0, r1, k))); ++nm; }
        } else {      // an INSERT cell: its own base is an M, the inserted bases follow it
            m_cell(byte_of(r0, r1, n));
            const uint32_t ins = c == t.hi ? t.tail : truth_ins_len(h, c);
            nm += ins; q += ins; ++c;
        }
    }
    num(run);
    return nm;
}
DW_DEV uint32_t truth_sat32(uint64_t v) { return v > 0xffffffffull ? 0xffffffffu : (uint32_t)v; }

// what the length pass and the write pass both derive for a lane: its range of the launch, its pair and read end, where its FASTQ record lies
struct TruthLane {
    SegPtr sg; bool valid; int j; uint64_t pair_in, pair, e;
    uint32_t rs, qn; bool rec_ok; const uint8_t *text;      // the record's start in `text`, the length of its QNAME, and whether the index and the text agree
};
// The grid is that of the k_simulate launch (a.n_blocks blocks of a.sim_threads lanes, the range table laid out for them): lane = read end.
// REC = false (the depth without the truth SAM): no record index exists and none is looked at -- rec_ok says yes, the text fields stay empty.
template <bool REC = true>
DW_DEV TruthLane truth_lane(const SimArgs &a, const TruthArgs &t)
{
    TruthLane L;
    const int lpp = t.lpp, tid = (int)threadIdx.x;
    L.sg = as_constant(a.segs) + seg_of_block(as_constant(a.segs), a.n_seg, blockIdx.x);
    L.j = lpp == 2 ? (tid & 1) : 0;
    L.pair_in = (uint64_t)(blockIdx.x - L.sg->first_block) * (uint64_t)(a.sim_threads / lpp) + (uint64_t)(tid / lpp);
    L.valid = L.pair_in < L.sg->n_pairs;
    L.pair = L.sg->pair_off + L.pair_in;
    L.e = L.pair * (uint64_t)lpp + (uint64_t)L.j;
    L.rs = 0; L.qn = 0; L.rec_ok = false; L.text = nullptr;
    if (!L.valid) return L;
    if constexpr (!REC) { L.rec_ok = true; return L; }
    // BWA: end j is record `pair` of stream j, its name ends "/1" or "/2"; BFAST alone: record e of the one interleaved stream, no suffix
    const int q = t.bfast ? 0 : L.j;
    const uint64_t r = t.bfast ? L.e : L.pair;
    const uint32_t *rec = q ? t.rec[1] : t.rec[0];
    const uint64_t n_text = *(q ? t.src_bytes[1] : t.src_bytes[0]);
    const uint32_t rs = rec[r], re = rec[r + 1];
    const uint32_t s = (uint32_t)(L.j ? a.p.len[1] : a.p.len[0]), fixed = 2u * s + 6u + (t.bfast ? 0u : 2u);      // '@' name [/1] \n seq \n + \n qual \n
    L.text = q ? t.src[1] : t.src[0];
    L.rec_ok = rs < re && (uint64_t)re <= n_text && re - rs > fixed && re - rs - fixed <= (uint32_t)t.qname_max && L.text[rs] == '@';
    L.rs = rs; L.qn = L.rec_ok ? re - rs - fixed : 0u;
    return L;
}
DW_DEV uint32_t truth_flag(const TruthArgs &t, int j, uint32_t f, uint32_t mate_f)      // f: TRUTH_F_* of the end and of its mate
{
    uint32_t flag = t.lpp == 2 ? (1u | (j ? 0x80u : 0x40u)) : 0u;
    if (f & TRUTH_F_RAND) return flag | 4u | (t.lpp == 2 ? 8u : 0u);
    if (t.lpp == 2) flag |= 2u | ((mate_f & TRUTH_F_REV) ? 0x20u : 0u);
    return flag | ((f & TRUTH_F_REV) ? 0x10u : 0u);
}
// TLEN of a mapped pair: rightmost end minus leftmost start plus one, positive for the leftmost end (end 1 on a tie)
DW_DEV int32_t truth_tlen(const TruthEnd &me, const TruthEnd &mate, int j)
{
    const int32_t lo = me.lo < mate.lo ? me.lo : mate.lo, hi = me.hi > mate.hi ? me.hi : mate.hi, span = hi - lo + 1;
    const bool first = me.lo < mate.lo || (me.lo == mate.lo && j == 0);
    return first ? span : -span;
}

// The length pass.  Reads meta, which belongs to the context and is overwritten by the next batch's k_simulate: the step runs on the stream of the
// launches, behind this batch's and in front of the next one's.
// <false, false>: the same replay where there is no FASTQ record to look at (the depth without the truth SAM: launch_truth_depth)
template <bool MD, bool REC = true>
__global__ void __launch_bounds__(SIM_THREADS) k_truth_len(SimArgs a, TruthArgs t)
{
    static_assert(REC || !MD, "the tags are read off the FASTQ record");
    const TruthLane L = truth_lane<REC>(a, t);
    if (!L.valid) return;
    const SegCtx sc = seg_ctx(a, L.sg);
    const uint32_t m = a.meta[L.pair];
    const int s = L.j ? a.p.len[1] : a.p.len[0];
    TruthEnd E; E.lo = E.hi = 0; E.lead = E.tail = 0; E.flags = 0; E.cigar = 0;
    if constexpr (MD) E.nm = E.md = 0;
    bool ok = L.rec_ok;
    if constexpr (MD) if (L.qn < TRUTH_MD_QNAME_MIN) ok = false;      // (truth_tags reads up to fifteen bytes in front of the bases)
    if (m & 0x80000000u) E.flags = TRUTH_F_RAND;
    else {
        const RngKey key{a.p.seed, L.sg->contig_index};
        const PairDraw pd = draw_pair(a, sc, key, L.sg->first_ii + L.pair_in, m & 0x3fffffffu);
        int64_t start; int step;
        read_geom(a, sc, pd, L.j, &start, &step);
        const HapDev h = sel_hap(a, sc, pd.hap);
        if (pd.is_rand || !truth_travel(h, (int32_t)sc.l, start, step, s, E)) ok = false;
        else {
            E.flags = (step < 0 ? TRUTH_F_REV : 0u) | (pd.hap ? TRUTH_F_HAP2 : 0u);
            uint32_t chars = 0;
            truth_cigar(h, E, [&](uint32_t n, uint32_t) { chars += truth_ndigits(n) + 1u; });
            E.cigar = chars;
            if constexpr (MD) if (ok) {
                uint32_t md = 0;
                E.nm = truth_tags(h, t.ref + sc.start, E, L.text + L.rs + 1u + L.qn + (t.bfast ? 0u : 2u) + 1u, (uint32_t)s, step < 0, [&](uint32_t n) { md += truth_ndigits(n); }, [&](uint32_t) { ++md; });
                E.md = md;
            }
        }
    }
    if (!ok) { E.flags |= TRUTH_F_BAD; atomicOr((unsigned long long *)&a.counters[STATUS_COUNTER], TRUTH_ERR_BIT); }
    t.ends[L.e] = E;
}
// The bytes of a line.  FLAG, PNEXT and TLEN need the mate's record, so the lengths are taken by a pass of their own behind k_truth_len: one lane per read end again
template <bool MD>
DW_DEV uint32_t truth_line_bytes(const SimArgs &a, const TruthArgs &t, const TruthLane &L, const TruthEnd &me, const TruthEnd &mate)
{
    const uint32_t s = (uint32_t)(L.j ? a.p.len[1] : a.p.len[0]);
    const uint32_t flag = truth_flag(t, L.j, me.flags, mate.flags);
    uint32_t n = L.qn + 1u + truth_ndigits(flag) + 1u;
    if (me.flags & TRUTH_F_RAND) n += 2u + 2u + 2u + 2u + 2u + 2u + 2u;      // * 0 0 * * 0 0, a tab behind each
    else {
        n += (uint32_t)(L.sg->name_fixed_len - t.prefix_len) + 1u + truth_ndigits((uint32_t)me.lo + 1u) + 1u + 3u + me.cigar + 1u;      // RNAME POS 60 CIGAR
        if (t.lpp == 2) { const int32_t tl = truth_tlen(me, mate, L.j); n += 2u + truth_ndigits((uint32_t)mate.lo + 1u) + 1u + (tl < 0 ? 1u : 0u) + truth_ndigits((uint32_t)(tl < 0 ? -tl : tl)) + 1u; }
        else n += 2u + 2u + 2u;                                                  // * 0 0
    }
    n += s + 1u + s;
    if (!(me.flags & TRUTH_F_RAND)) n += 7u;                                      // \t HP:i:1
    if constexpr (MD) if (!(me.flags & TRUTH_F_RAND)) n += 6u + truth_ndigits(me.nm) + 6u + me.md;      // \t NM:i: n \t MD:Z: string
    return n + 1u;
}
// ... scanned inside the block at once (the lanes of a block are consecutive read ends): line_len[e] = the bytes of the block's lines in front of line e,
// blk[block] = the block's bytes; k_scan_excl over the blocks does the rest (one block scanning every line of a 2^18-pair batch took as long as two k_simulate)
// <true>: a tagged line spells out every deleted base, so no bound in the read length holds for it: the block's sums are taken in 64 bits (two scans of 16 bits
// each) and stored saturated -- 0xffffffff lies behind every buffer the host can make
template <bool MD>
__global__ void __launch_bounds__(SIM_THREADS) k_truth_len2(SimArgs a, TruthArgs t)
{
    __shared__ uint32_t sm[17];
    const TruthLane L = truth_lane(a, t);
    uint32_t len = 0;
    if (L.valid) {
        const TruthEnd me = t.ends[L.e], mate = t.lpp == 2 ? t.ends[L.e ^ 1ull] : me;
        if (!((me.flags | mate.flags) & TRUTH_F_BAD)) len = truth_line_bytes<MD>(a, t, L, me, mate);      // (a pair's lines stand or fall together)
    }
    if constexpr (!MD) {
        uint32_t total;
        const uint32_t before = block_excl_scan(len, sm, &total);      // (every lane of the block takes part)
        if (L.valid) t.line_len[L.e] = before;
        if (threadIdx.x == 0) t.blk[blockIdx.x] = total;
    } else {
        uint32_t tl, th;
        const uint32_t bl = block_excl_scan(len & 0xffffu, sm, &tl), bh = block_excl_scan(len >> 16, sm, &th);
        if (L.valid) t.line_len[L.e] = truth_sat32((uint64_t)bl + ((uint64_t)bh << 16));
        if (threadIdx.x == 0) t.blk[blockIdx.x] = truth_sat32((uint64_t)tl + ((uint64_t)th << 16));
    }
}
// k_scan_excl for the blocks' bytes of tagged lines: the running sum in 64 bits, the prefixes stored saturated.  *total_out is exact unless a block's own sum
// was saturated -- and then it is 2^32 - 1 at least, which the host refuses.  *fit_out: what the gzip kernel may read of the text, nothing where it did not fit
__global__ void __launch_bounds__(1024) k_truth_scan(uint32_t *data, uint32_t n, uint64_t *total_out, uint64_t cap, uint64_t *fit_out)
{
    __shared__ uint32_t sm[17];
    uint64_t grand = 0;
    for (uint32_t base = 0; base < n; base += 1024u) {
        const uint32_t i = base + threadIdx.x, v = i < n ? data[i] : 0u;
        uint32_t tl, th;
        const uint32_t bl = block_excl_scan(v & 0xffffu, sm, &tl), bh = block_excl_scan(v >> 16, sm, &th);
        if (i < n) data[i] = truth_sat32(grand + (uint64_t)bl + ((uint64_t)bh << 16));
        grand += (uint64_t)tl + ((uint64_t)th << 16);
    }
    if (threadIdx.x == 0) { *total_out = grand; *fit_out = grand <= cap ? grand : 0ull; }
}

// `n` bytes from src, in order or -- turn -- last byte first, each through the complement where comp is set
template <class O>
DW_DEV void truth_copy(O &o, const uint8_t *src, uint32_t n, bool turn, bool comp)
{
    auto cb = [&](uint32_t b) -> uint32_t {
        if (!comp) return b;
        return b == 'A' ? (uint32_t)'T' : b == 'T' ? (uint32_t)'A' : b == 'C' ? (uint32_t)'G' : b == 'G' ? (uint32_t)'C' : b;
    };
    uint32_t k = 0;
    for (; k + 8 <= n; k += 8) {
        uint64_t v = reinterpret_cast<const Unal8 *>(turn ? src + (n - 8 - k) : src + k)->v;
        if (turn) v = __builtin_bswap64(v);
        if (comp) { uint64_t w = 0; for (int q = 0; q < 8; ++q) w |= (uint64_t)cb((uint32_t)(v >> (8 * q)) & 0xffu) << (8 * q); v = w; }
        o.putn(v, 8);
    }
    for (; k < n; ++k) o.put(cb(turn ? src[n - 1 - k] : src[k]));
}
// The write pass: a line starts at blk[block] (scanned) + line_len[e]; the text's length stands in *t.total.  A line is written only if it ends inside the buffer (the host
// sized it from a proven bound: a belt to its braces).  <true>: no such bound (a deletion's bases are spelled out), so a line that would end behind the buffer is
// left out under a status bit of its own, TRUTH_ROOM_BIT: the host runs the batch again with the room *t.total asks for.
template <bool MD>
__global__ void __launch_bounds__(SIM_THREADS) k_truth_write(SimArgs a, TruthArgs t)
{
    const TruthLane L = truth_lane(a, t);
    if (!L.valid) return;
    const TruthEnd me = t.ends[L.e], mate = t.lpp == 2 ? t.ends[L.e ^ 1ull] : me;
    if ((me.flags | mate.flags) & TRUTH_F_BAD) return;
    const uint32_t len = truth_line_bytes<MD>(a, t, L, me, mate);
    const uint64_t off = (uint64_t)t.blk[blockIdx.x] + t.line_len[L.e];
    if (off + len > t.cap) { atomicOr((unsigned long long *)&a.counters[STATUS_COUNTER], MD ? TRUTH_ROOM_BIT : TRUTH_ERR_BIT); return; }
    const uint32_t s = (uint32_t)(L.j ? a.p.len[1] : a.p.len[0]);
    const bool rnd = (me.flags & TRUTH_F_RAND) != 0, rev = !rnd && (me.flags & TRUTH_F_REV);
    Writer o; o.init(t.out + off);
    const uint8_t *rec = L.text + L.rs;
    truth_copy(o, rec + 1, L.qn, false, false);
    o.put('\t'); truth_put_dec(o, truth_flag(t, L.j, me.flags, mate.flags)); o.put('\t');
    if (rnd) truth_lit(o, "*\t0\t0\t*\t*\t0\t0\t");
    else {
        const SegCtx sc = seg_ctx(a, L.sg);
        const HapDev h = sel_hap(a, sc, (me.flags & TRUTH_F_HAP2) ? 1 : 0);
        truth_copy(o, a.names + L.sg->name_off + 1 + t.prefix_len, (uint32_t)(L.sg->name_fixed_len - t.prefix_len), false, false);
        o.put('\t'); truth_put_dec(o, (uint32_t)me.lo + 1u); truth_lit(o, "\t60\t");
        truth_cigar(h, me, [&](uint32_t n, uint32_t letter) { truth_put_dec(o, n); o.put(letter); });
        o.put('\t');
        if (t.lpp == 2) {
            const int32_t tl = truth_tlen(me, mate, L.j);
            truth_lit(o, "=\t"); truth_put_dec(o, (uint32_t)mate.lo + 1u); o.put('\t');
            if (tl < 0) o.put('-');
            truth_put_dec(o, (uint32_t)(tl < 0 ? -tl : tl)); o.put('\t');
        } else truth_lit(o, "*\t0\t0\t");
    }
    const uint8_t *seq = rec + 1 + L.qn + (t.bfast ? 0u : 2u) + 1u;
    truth_copy(o, seq, s, rev, rev);
    o.put('\t');
    truth_copy(o, seq + s + 3u, s, rev, false);
    if (!rnd) { truth_lit(o, "\tHP:i:"); o.put((me.flags & TRUTH_F_HAP2) ? '2' : '1'); }
    if constexpr (MD) if (!rnd) {      // the second walk of the tags: no MD string is ever stored between the passes
        const SegCtx sc = seg_ctx(a, L.sg);
        const HapDev h = sel_hap(a, sc, (me.flags & TRUTH_F_HAP2) ? 1 : 0);
        truth_lit(o, "\tNM:i:"); truth_put_dec(o, me.nm); truth_lit(o, "\tMD:Z:");
        (void)truth_tags(h, t.ref + sc.start, me, seq, s, rev, [&](uint32_t n) { truth_put_dec(o, n); }, [&](uint32_t c) { o.put(c); });
    }
    o.put('\n');
    o.flush();
}

// ---- the true read depth of every listed mutated cell (dwgsim_hip_set_truth_depth; DESIGN.md "6f") ----
// THE RULE.  Per listed cell p of the group (DepthArgs::pos: every cell that is mutated on either haplotype, ascending) there are two 64-bit counters, n[1] and
// n[2].  A mapped read end of haplotype h whose alignment is the cells lo .. hi with `tail` inserted bases behind hi's own (TruthEnd, as k_truth_len left it)
// adds 1 to n[h] of every listed cell p with lo <= p <= hi -- except that where haplotype h carries an insertion at p and p == hi the end counts only if
// `tail` is the insertion's full length: it then holds the cell's own base AND every inserted base, anything less does not show the variant.
// What follows from the replay law above needs no case of its own: lo and hi are never deleted cells and a CIGAR never starts or ends with D, so a deleted cell
// inside lo .. hi is a deletion the read spans completely (the first cell of a deleted run stands for the run in the VCF record); a `lead` never counts (the
// cell it belongs to lies left of lo and its own base is not in the read); random ends (TRUTH_F_RAND) and ends without a line (TRUTH_F_BAD) count nowhere.
// Sequencing errors are not looked at: this is the depth by ORIGIN of the read, not by the base it shows.
// One lane per read end on the grid of the launch, behind k_truth_len.  Most ends hold no listed cell at all (at the default rate one 150-base end in seven
// does), so the search is what every lane pays: a lower bound without a branch, the same number of steps in every lane (it depends on the list's length
// alone), then the walk over the few cells in reach -- the only divergent part -- with one 64-bit atomicAdd each.  Integer adds commute: the counters do
// not depend on the order of lanes, blocks, batches or devices.
DW_DEV uint32_t depth_lower_bound(const int32_t *pos, uint32_t n, int32_t key)      // the first e with pos[e] >= key (n: none)
{
    uint32_t base = 0, len = n;
    while (len > 1u) { const uint32_t half = len >> 1; base += pos[base + half - 1u] < key ? half : 0u; len -= half; }
    return base + (len == 1u && pos[base] < key ? 1u : 0u);
}
__global__ void __launch_bounds__(SIM_THREADS) k_truth_depth(SimArgs a, TruthArgs t, DepthArgs d)
{
    const TruthLane L = truth_lane<false>(a, t);
    if (!L.valid || d.n == 0u) return;
    const TruthEnd E = t.ends[L.e];
    if (E.flags & (TRUTH_F_RAND | TRUTH_F_BAD)) return;
    const SegCtx sc = seg_ctx(a, L.sg);
    const int hap = (E.flags & TRUTH_F_HAP2) ? 1 : 0;
    const int32_t glo = (int32_t)sc.start + E.lo, ghi = (int32_t)sc.start + E.hi;      // the list holds group coordinates
    for (uint32_t e = depth_lower_bound(d.pos, d.n, glo); e < d.n; ++e) {
        const int32_t p = d.pos[e];
        if (p > ghi) break;
        if (p == ghi) {      // (E.hi lies inside the contig: h.cells is the contig's)
            const HapDev h = sel_hap(a, sc, hap);
            if ((h.cells[E.hi] & TMASK) == T_INS && E.tail != truth_ins_len(h, E.hi)) break;
        }
        atomicAdd(&d.cnt[2u * e + (uint32_t)hap], 1ull);
    }
}

// The step, enqueued behind the k_simulate launch whose arguments `a` are (and the k_split_scan / look-backs that leave the text lengths in its counters)
// depth: the counters of the true read depth are taken behind the length pass (nullptr: not)
void launch_truth(hipStream_t st, const SimArgs &a, const TruthArgs &t, const DepthArgs *depth)
{
    const int n_src = t.bfast ? 1 : t.lpp;
    for (int q = 0; q < n_src; ++q) {
        const uint32_t nb = cdiv(t.src_cap[q], TRUTH_NL_BYTES);
        if (nb == 0) continue;
        hipLaunchKernelGGL(k_truth_nl_count, dim3(nb), dim3(TRUTH_NL_THREADS), 0, st, t.src[q], t.src_bytes[q], t.nl_count[q]);
        launch_scan_excl(st, t.nl_count[q], nb, nullptr);
        hipLaunchKernelGGL(k_truth_nl_index, dim3(nb), dim3(TRUTH_NL_THREADS), 0, st, t.src[q], t.src_bytes[q], t.nl_count[q], t.rec[q], t.n_rec[q]);
    }
    if (t.md) {
        hipLaunchKernelGGL(k_truth_len<true>, dim3(a.n_blocks), dim3(a.sim_threads), 0, st, a, t);
        if (depth) hipLaunchKernelGGL(k_truth_depth, dim3(a.n_blocks), dim3(a.sim_threads), 0, st, a, t, *depth);
        hipLaunchKernelGGL(k_truth_len2<true>, dim3(a.n_blocks), dim3(a.sim_threads), 0, st, a, t);
        hipLaunchKernelGGL(k_truth_scan, dim3(1), dim3(1024), 0, st, t.blk, a.n_blocks, t.total, t.cap, t.fit);
        hipLaunchKernelGGL(k_truth_write<true>, dim3(a.n_blocks), dim3(a.sim_threads), 0, st, a, t);
        return;
    }
    hipLaunchKernelGGL(k_truth_len<false>, dim3(a.n_blocks), dim3(a.sim_threads), 0, st, a, t);
    if (depth) hipLaunchKernelGGL(k_truth_depth, dim3(a.n_blocks), dim3(a.sim_threads), 0, st, a, t, *depth);
    hipLaunchKernelGGL(k_truth_len2<false>, dim3(a.n_blocks), dim3(a.sim_threads), 0, st, a, t);
    launch_scan_excl(st, t.blk, a.n_blocks, t.total);
    hipLaunchKernelGGL(k_truth_write<false>, dim3(a.n_blocks), dim3(a.sim_threads), 0, st, a, t);
}
// The depth without the truth SAM: the replay and the counters, nothing else -- no record index, no lengths, no scan, no text (t: lpp and ends alone)
void launch_truth_depth(hipStream_t st, const SimArgs &a, const TruthArgs &t, const DepthArgs &depth)
{
    hipLaunchKernelGGL((k_truth_len<false, false>), dim3(a.n_blocks), dim3(a.sim_threads), 0, st, a, t);
    hipLaunchKernelGGL(k_truth_depth, dim3(a.n_blocks), dim3(a.sim_threads), 0, st, a, t, depth);
}

} // namespace dw
