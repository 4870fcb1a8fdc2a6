"""The DEFLATE stream of k_gzip (dwgsim_amd/csrc/dw_gzip.hip) held against a reference of the test's own -- shared by tests/test_emu_gzip_stream.py
(the kernel's source on the CPU emulation) and tests/test_gpu_gzip_stream.py (the device).  A decoder accepts any valid stream; what is checked here is
the stream the kernel was WRITTEN to make: complete codes, optimal code lengths (Huffman by a heap; package-merge where 15 bits bind), the run-length
coded block header, the shape of a member, where the matches lie and what they save, and that the same text gives the same bytes.

Nothing here shares a method with the kernel: the reader walks the bits one code at a time through a lookup table, the optimal costs come from a heap
and from package-merge, the header's bits are counted run by run from the decoded lengths."""
import functools
import hashlib
import heapq
import json
import os
import random
import zlib

from dwgsim_amd import api

CHUNK, SPAN, MAX_MATCHES_PER_SPAN, IMAGE = 32768, 128, 8, 24576      # a member's text, a lane's share of it, matches kept per share, the member image (bytes)
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_FILE = os.path.join(HERE, "golden", "gzip_members.json")


class StreamError(ValueError):
    """what zlib would reject too"""


# ---------------------------------------------------------------- the reader ----------------------------------------------------------------
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DL = [5] * 32            # (30 and 31 take part in the fixed code and never occur)


def kraft(lens):
    """sum of 2^(15 - l) over the used lengths: 2^15 for a complete code"""
    return sum(1 << (15 - l) for l in lens if l)


def decode_table(lens, what, may_be_short):
    """(table, bits): table[the next `bits` bits of the stream, LSB first] = symbol << 4 | length, 0 where no code starts.  Rejects what zlib's
    inflate_table rejects: an over-subscribed set always; an incomplete one unless it is a single code of length 1 of the literal / length or
    distance alphabet (`may_be_short`)."""
    if any(l > 15 for l in lens):
        raise StreamError(f"{what}: a code longer than 15 bits")
    used = [l for l in lens if l]
    if not used:
        return [0, 0], 1
    k = kraft(used)
    if k > 1 << 15:
        raise StreamError(f"{what}: over-subscribed code lengths")
    if k < 1 << 15 and not (may_be_short and max(used) == 1):
        raise StreamError(f"{what}: incomplete code lengths")
    bits = max(used)
    count = [0] * 17
    for l in used:
        count[l] += 1
    nxt, c = [0] * 17, 0
    for b in range(1, 16):
        c = (c + count[b - 1]) << 1
        nxt[b] = c
    table = [0] * (1 << bits)
    for s, l in enumerate(lens):
        if l:
            c = nxt[l]; nxt[l] += 1
            r = int(format(c, "0%db" % l)[::-1], 2)
            table[r::1 << l] = [s << 4 | l] * (1 << (bits - l))
    return table, bits


class _Bits:
    def __init__(self, b, byte_pos):
        self.b, self.p, self.acc, self.nb = b, byte_pos, 0, 0       # p: the next byte to load; acc holds nb bits not yet consumed

    def need(self, n):
        while self.nb < n:
            piece = self.b[self.p:self.p + 8]
            if not piece:
                raise StreamError("the stream ends inside a block")
            self.acc |= int.from_bytes(piece, "little") << self.nb
            self.nb += 8 * len(piece); self.p += len(piece)

    def get(self, n):
        if n == 0:
            return 0
        self.need(n)
        v = self.acc & ((1 << n) - 1)
        self.acc >>= n; self.nb -= n
        return v

    def sym(self, table, bits, what):
        try:
            self.need(bits)
        except StreamError:
            if self.nb == 0:
                raise
        e = table[self.acc & ((1 << bits) - 1)]
        if e == 0 or (e & 15) > self.nb:
            raise StreamError(f"{what}: no such code")
        self.acc >>= e & 15; self.nb -= e & 15
        return e >> 4

    def pos(self):
        return 8 * self.p - self.nb

    def to_byte(self):
        drop = self.nb & 7
        self.acc >>= drop; self.nb -= drop
        return self.pos() >> 3


def read_member(b, off=0):
    """One gzip member (RFC 1952) at b[off:], inflated bit by bit (RFC 1951).  Returns a dict:
         header   the ten fixed bytes            pad     the FNAME field without its NUL (None where FLG has no FNAME)
         blocks   [block]                        out     the decompressed bytes
         size     bytes of the member            crc, isize   as stored (both verified here)
       a stored block:  type 0, final, len
       a coded block:   type 1 (fixed) or 2 (dynamic), final, ll / dl (the code lengths of both alphabets), tokens (a literal as an int, a match as
                        (position in the member's text, length, distance)), lh / dh (how often every literal / length and distance symbol was coded,
                        end-of-block included), data_bits (the codes, end-of-block included), max_token_bits;
                        dynamic only: hlit, hdist, hclen, cl (the 19 code-length code lengths), hdr_bits (from BFINAL to the last coded length)"""
    if b[off:off + 3] != b"\x1f\x8b\x08":
        raise StreamError("not a gzip member")
    flg, p = b[off + 3], off + 10
    if flg & 0xE0:
        raise StreamError("reserved flag bits")
    if flg & 4:
        p += 2 + int.from_bytes(b[p:p + 2], "little")
    pad = None
    if flg & 8:
        q = b.index(b"\0", p)
        pad, p = bytes(b[p:q]), q + 1
    if flg & 16:
        p = b.index(b"\0", p) + 1
    if flg & 2:
        p += 2
    bs, out, blocks = _Bits(b, p), bytearray(), []
    while True:
        h0 = bs.pos()
        final, typ = bs.get(1), bs.get(2)
        if typ == 0:
            q = bs.to_byte()
            ln, nln = bs.get(16), bs.get(16)
            if ln ^ nln != 0xFFFF:
                raise StreamError("stored block: LEN and NLEN do not agree")
            q = bs.to_byte()
            assert bs.nb % 8 == 0
            if q + ln > len(b):
                raise StreamError("the stream ends inside a stored block")
            out += b[q:q + ln]
            bs = _Bits(b, q + ln)
            blocks.append(dict(type=0, final=final, len=ln))
        elif typ == 3:
            raise StreamError("block type 3")
        else:
            blk = dict(type=typ, final=final)
            if typ == 2:
                hlit, hdist, hclen = bs.get(5) + 257, bs.get(5) + 1, bs.get(4) + 4
                if hlit > 286 or hdist > 30:
                    raise StreamError("too many length or distance symbols")
                cl = [0] * 19
                for i in range(hclen):
                    cl[CL_ORDER[i]] = bs.get(3)
                ct, cb = decode_table(cl, "code-length code", False)
                lens = []
                while len(lens) < hlit + hdist:
                    s = bs.sym(ct, cb, "code-length code")
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        if not lens:
                            raise StreamError("repeat with no length before it")
                        lens += [lens[-1]] * (3 + bs.get(2))
                    elif s == 17:
                        lens += [0] * (3 + bs.get(3))
                    else:
                        lens += [0] * (11 + bs.get(7))
                if len(lens) != hlit + hdist:
                    raise StreamError("a repeat runs past the last code length")
                ll, dl = lens[:hlit], lens[hlit:]
                if ll[256] == 0:
                    raise StreamError("no end-of-block code")
                blk.update(hlit=hlit, hdist=hdist, hclen=hclen, cl=cl, hdr_bits=bs.pos() - h0)
            else:
                ll, dl = FIXED_LL, FIXED_DL
            lt, lb = decode_table(ll, "literal / length code", True)
            dt, db = decode_table(dl, "distance code", True)
            lmask, dmask = (1 << lb) - 1, (1 << db) - 1
            tokens, lh, dh, d0, widest = [], [0] * 288, [0] * 32, bs.pos(), 0
            acc, nb, p, n_b = bs.acc, bs.nb, bs.p, len(b)
            while True:
                if nb < 48:                                        # the widest token: 15 + 5 + 15 + 13 bits
                    piece = b[p:p + 8]
                    acc |= int.from_bytes(piece, "little") << nb
                    nb += 8 * len(piece); p += len(piece)
                e = lt[acc & lmask]
                l = e & 15
                if e == 0 or l > nb:
                    raise StreamError("literal / length code: no such code, or the stream ends inside a block")
                acc >>= l; nb -= l
                s = e >> 4
                lh[s] += 1
                if s < 256:
                    out.append(s); tokens.append(s)
                elif s == 256:
                    break
                else:
                    if s > 285:
                        raise StreamError("length symbol 286 or 287")
                    x = LEN_EXTRA[s - 257]
                    length = LEN_BASE[s - 257] + (acc & ((1 << x) - 1))
                    acc >>= x; nb -= x
                    e = dt[acc & dmask]
                    l2 = e & 15
                    if e == 0 or l2 > nb:
                        raise StreamError("distance code: no such code")
                    acc >>= l2; nb -= l2
                    ds = e >> 4
                    if ds > 29:
                        raise StreamError("distance symbol 30 or 31")
                    dh[ds] += 1
                    y = DIST_EXTRA[ds]
                    dist = DIST_BASE[ds] + (acc & ((1 << y) - 1))
                    acc >>= y; nb -= y
                    if nb < 0:
                        raise StreamError("the stream ends inside a block")
                    if dist > len(out):
                        raise StreamError("a distance before the start of the member")
                    widest = max(widest, l + x + l2 + y)
                    tokens.append((len(out), length, dist))
                    for _ in range(length):
                        out.append(out[-dist])
            bs.acc, bs.nb, bs.p = acc, nb, p
            if typ == 1:
                ll = list(FIXED_LL)
            blk.update(ll=ll, dl=list(dl), tokens=tokens, lh=lh[:286], dh=dh[:30], data_bits=bs.pos() - d0, max_token_bits=widest)
            blocks.append(blk)
        if final:
            break
    q = bs.to_byte()
    if q + 8 > len(b):
        raise StreamError("the stream ends before CRC and ISIZE")
    crc, isize = int.from_bytes(b[q:q + 4], "little"), int.from_bytes(b[q + 4:q + 8], "little")
    if crc != zlib.crc32(bytes(out)):
        raise StreamError("CRC-32 does not match")
    if isize != len(out) & 0xFFFFFFFF:
        raise StreamError("ISIZE does not match")
    return dict(header=bytes(b[off:off + 10]), pad=pad, blocks=blocks, out=bytes(out), size=q + 8 - off, crc=crc, isize=isize)


def read_members(gz):
    out, off = [], 0
    while off < len(gz):
        m = read_member(gz, off)
        out.append(m); off += m["size"]
    return out


# ---------------------------------------------------------------- optimal code costs ----------------------------------------------------------------
def huffman(hist):
    """(cost in bits, depth) of an unlimited Huffman code of the non-zero counts; among equal weights the shallower tree is merged first, which gives the
    least deep of the optimal trees.  A single used symbol takes one bit (RFC 1951: one distance code is sent with one bit)."""
    hp = [(w, 0) for w in hist if w]
    if len(hp) < 2:
        return (hp[0][0], 1) if hp else (0, 0)
    heapq.heapify(hp)
    cost = 0
    while len(hp) > 1:
        a, b = heapq.heappop(hp), heapq.heappop(hp)
        cost += a[0] + b[0]
        heapq.heappush(hp, (a[0] + b[0], max(a[1], b[1]) + 1))
    return cost, hp[0][1]


def package_merge(hist, limit=15):
    """cost in bits of an optimal code with no length over `limit` (Larmore and Hirschberg's package-merge, the plain form)"""
    leaves = sorted((w, (i,)) for i, w in enumerate(hist) if w)
    n = len(leaves)
    if n < 2:
        return leaves[0][0] if n else 0
    assert n <= 1 << limit
    pk = list(leaves)
    for _ in range(limit - 1):
        merged = [(pk[i][0] + pk[i + 1][0], pk[i][1] + pk[i + 1][1]) for i in range(0, len(pk) - 1, 2)]
        pk = sorted(leaves + merged, key=lambda x: x[0])
    length = {}
    for _, syms in pk[:2 * n - 2]:
        for i in syms:
            length[i] = length.get(i, 0) + 1
    return sum(hist[i] * l for i, l in length.items())


def literal_histogram(data):
    """counts of the bytes of data as literals, and end-of-block once"""
    import numpy as np
    return [int(c) for c in np.bincount(np.frombuffer(data, dtype=np.uint8), minlength=256)] + [1]


# ---------------------------------------------------------------- the block header's bits ----------------------------------------------------------------
def _cl_bits(sym):
    return 4 if sym <= 12 else 5           # the kernel's fixed code-length code


def _runs(seq):
    i = 0
    while i < len(seq):
        j = i
        while j < len(seq) and seq[j] == seq[i]:
            j += 1
        yield seq[i], j - i
        i = j


def header_bits_reference(ll, dl):
    """bits of a dynamic block's header from BFINAL to the last code length, coded run by run (the two alphabets apart): a run of a non-zero length is the
    length, then symbol 16 for groups of up to 6 and what is left under 3 written out; a run of zeros is symbol 18 for groups of up to 138 while 11 or
    more are left, then symbol 17 for 3 or more, else zeros"""
    bits = 3 + 5 + 5 + 4 + 19 * 3
    for seq in (ll, dl):
        for v, run in _runs(seq):
            if v:
                bits += _cl_bits(v); run -= 1
                while run >= 3:
                    r = min(run, 6)
                    bits += _cl_bits(16) + 2; run -= r
                bits += run * _cl_bits(v)
            else:
                while run >= 11:
                    r = min(run, 138)
                    bits += _cl_bits(18) + 7; run -= r
                if run >= 3:
                    bits += _cl_bits(17) + 3; run = 0
                bits += run * _cl_bits(0)
    return bits


# ---------------------------------------------------------------- inputs ----------------------------------------------------------------
def fastq_like(rng, n_bytes):
    """FASTQ-like text of n_bytes: one of eight styles (CRLF, read lengths that vary, contig names that change, names of two letters, names that are a
    repeated contig name, quality and base lines that look like name and separator lines, "+name" separators), quality alphabets with '@' and '+',
    read lengths 0 .. 400, names of 1 .. 200 bytes; a third of the streams start mid-record; the cut at n_bytes leaves no trailing newline"""
    style = rng.randrange(8)
    out, idx = bytearray(), rng.randrange(10 ** rng.randrange(1, 9))
    ctg = bytes(rng.choice(b"abcXYZ_01") for _ in range(rng.choice([1, 3, 8, 20, 70, 150])))
    qa = rng.choice([b"IIIIIIIH", b"@+IJ#", bytes(range(33, 74)), b"@", b"+@"])
    L = rng.choice([0, 1, 2, 5, 17, 36, 50, 100, 150, 250, 400])
    nl = b"\r\n" if style == 1 else b"\n"
    while len(out) < n_bytes:
        l = L if style != 2 else rng.randrange(0, 2 * L + 1)
        if style == 3 and rng.random() < 0.1:
            ctg = bytes(rng.choice(b"abcXYZ_01") for _ in range(rng.randrange(1, 100)))
        p1 = rng.randrange(1, 10 ** rng.randrange(1, 9)); p2 = p1 + rng.randrange(600)
        name = b"@" + ctg + b"_%d_%d_%d_%d_0_0_%d:0:0_%d:0:0_%x/1" % (p1, p2, rng.randrange(2), rng.randrange(2), rng.randrange(3), rng.randrange(3), idx)
        idx += 1
        if style == 4:
            name = b"@" + bytes(rng.choice(b"AB") for _ in range(rng.randrange(3, 90)))
        if style == 5:
            name = b"@" + ctg * rng.randrange(1, 4)
        name = name[:200]
        seq = bytes(rng.choice(b"ACGTN") for _ in range(l)); q = bytes(rng.choice(qa) for _ in range(l))
        if style == 6:
            q = b"@" + q; seq = b"+" + seq
        plus = b"+" if style != 7 else b"+" + name[1:]
        out += name + nl + seq + nl + plus + nl + q + nl
    out = out[:n_bytes]
    if rng.random() < 0.3 and out:
        out = out[rng.randrange(0, min(300, len(out))):]
    return bytes(out)


def fuzz_inputs(seed, n):
    rng = random.Random(seed)
    for _ in range(n):
        size = rng.choice([rng.randrange(1, 400), rng.randrange(CHUNK - 200, CHUNK + 200), rng.randrange(1, 70000), 65536 + rng.randrange(-3, 4)])
        yield fastq_like(rng, size)


def chain_weights(n_bytes_symbols):
    """byte counts 1, 1, 3, 4, 7, 11, 18, 29, ...: with end-of-block's 1 in front, every weight is one more than the sum of all weights before the last --
    the node the two-queue merge has built two steps back -- so the merge never leaves the chain, whatever the tie rule, and n byte symbols give a code n deep
    (n >= 2)"""
    allw = [1, 1, 1]                      # end of block, then the bytes
    while len(allw) < n_bytes_symbols + 1:
        allw.append(sum(allw) - allw[-1] + 1)
    return allw[1:]


CHAINS = {3569: 16, 5776: 17, 15125: 19, 24474: 20}      # bytes of the input: depth of its unlimited Huffman code (3 569: the smallest input that needs the limit)
CHAIN_ORDERS = ("sorted", "shuffled", "rarest-first")


def chain_input(n_bytes, order):
    for n in range(2, 40):
        w = chain_weights(n)
        if sum(w) == n_bytes:
            break
    else:
        raise AssertionError(n_bytes)
    data = bytearray(b"".join(bytes([40 + k]) * f for k, f in enumerate(w)))      # rarest first
    if order == "sorted":
        data.reverse()
    elif order == "shuffled":
        random.Random(n_bytes).shuffle(data)
    else:
        assert order == "rarest-first"
    return bytes(data)


@functools.lru_cache(None)
def _skewed_pool():
    fib = [1, 1]
    while len(fib) < 22:
        fib.append(fib[-1] + fib[-2])
    pool = bytearray(b"".join(bytes([65 + k]) * f for k, f in enumerate(fib)))
    random.Random(7).shuffle(pool)
    return bytes(pool)


LONG_RECORDS = {600: 120, 4100: 16, 8300: 8, 12000: 6, 16400: 6, 17000: 6, 20000: 5}      # length of a record: records
LONG_REACH = (8300, 12000, 16400, 17000, 20000)            # distances of 12 and 13 extra bits (symbols 26 .. 29)


def long_records(rec_len):
    """four-line records of rec_len bytes under one 50-byte name whose last five digits count up; bases and qualities from a skewed pool"""
    pool, out = _skewed_pool(), bytearray()
    for i in range(LONG_RECORDS[rec_len]):
        nm = (b"@q01234567" * 10)[:44] + b"%05d" % i
        body = (rec_len - len(nm) - 5) // 2
        s = pool[(i * body) % 20000:][:body]; s = s + pool[:body - len(s)]
        rec = nm + b"\n" + s + b"\n+\n" + s[::-1] + b"\n"
        out += rec
    return bytes(out)


def wide_token_input():
    """a length code made deep (15 bits) by chain counts, met by a distance near 16 400 (13 extra bits): a match token of more than 32 bits in the first member"""
    n_sym, scale, n_short = 15, 14, 24
    rng = random.Random(n_sym * 100 + scale + n_short)
    pool = bytearray(b"".join(bytes([70 + k]) * (f * scale) for k, f in enumerate(chain_weights(n_sym - 1))))
    rng.shuffle(pool)
    pool = bytes(pool) * 3
    out, pp = bytearray(), 0
    def rec(nm, body):
        nonlocal pp
        s = pool[pp:pp + body]; pp += body
        return nm + b"\n" + s + b"\n+\n" + s[::-1] + b"\n"
    for _ in range(n_short):
        a = bytes(rng.choice(b"FGHIJKL") for _ in range(7)); b = bytes(rng.choice(b"FGHIJKL") for _ in range(10))
        out += rec(b"@" + a * 3 + b * 3, 20)
    far = b"@" + bytes(rng.choice(b"FGHIJKLMNOP") for _ in range(50))
    for _ in range(3):
        out += rec(far, 8200)
    return bytes(out)


SIMULATED = [      # (name, FASTA, flags, pairs): stream 1 (stream 0 where stream 1 is empty), the first 64 KiB: two full members
    ("sim_150x2", "tiny.fa", "-z 9 -N 900 -1 150 -2 150 -y 0.1", 230),
    ("sim_36x2_prefix", "tiny.fa", "-z 3 -N 900 -1 36 -2 36 -d 100 -s 5 -P some_prefix", 600),
    ("sim_50_single", "tiny.fa", "-z 4 -N 900 -1 50 -2 0 -o 1", 800),
    ("sim_solid_50x2", "tiny.fa", "-z 5 -N 900 -c 1 -1 50 -2 50 -y 0.1", 500),
    ("sim_ex1_70x2", "ex1.fa", "-z 13 -N 900 -1 70 -2 70", 450),
    ("sim_ion_120", "odd.fa", "-z 6 -N 700 -c 2 -f TACGTACGTCTGAGCATCGATCGATGTACAGC -1 120 -2 0", 500),
]


def simulated_text(lib, golden_dir, fasta, flags, pairs):
    params = api.parse_flags(flags, lib)
    name, arr = api.read_fasta(os.path.join(golden_dir, fasta))[0]
    with api.Context(params, 0, lib) as ctx:
        cid = ctx.add_contig(name, arr, 0)
        ctx.mutate(cid)
        b = ctx.simulate(cid, 0, pairs, 0, 0)
        s = 1 if b.bytes[1] else 0
        txt = ctx.fetch(0, s, b.bytes[s])
    assert len(txt) >= 2 * CHUNK, (flags, len(txt))
    return txt[:2 * CHUNK]


GOLDEN_FUZZ_SEEDS = (101, 102, 103, 104, 105, 106, 107, 108)


# ---------------------------------------------------------------- the checks ----------------------------------------------------------------
class Session:
    """one context of `lib` and what it has compressed so far: name -> (text, members as bytes, members as read)"""

    def __init__(self, lib, golden_dir=None):
        self.lib, self.golden_dir = lib, golden_dir or os.path.join(HERE, "golden")
        self.ctx = api.Context(api.parse_flags("-z 9 -N 10", lib), 0, lib)
        self.done, self.texts = {}, {}
        self.stats = dict(members=0, stored=0, matches=0, flattened=0, worst_excess=0.0)

    def close(self):
        self.ctx.close()

    def named_input(self, name):
        if name not in self.texts:
            kind, _, arg = name.partition(":")
            if kind == "chain":
                n, order = arg.split("/")
                data = chain_input(int(n), order)
            elif kind == "long":
                data = long_records(int(arg))
            elif kind == "wide":
                data = wide_token_input()
            elif kind == "fuzz":
                data = next(fuzz_inputs(int(arg), 1))
            else:
                fasta, flags, pairs = next(c[1:] for c in SIMULATED if c[0] == name)
                data = simulated_text(self.lib, self.golden_dir, fasta, flags, pairs)
            self.texts[name] = data
        return self.texts[name]

    def compress(self, name, data=None):
        """the checked members of a named input (compressed once per session)"""
        if name not in self.done:
            data = self.named_input(name) if data is None else data
            gz = self.ctx.debug_gzip(data)
            self.done[name] = (data, gz, check_stream(data, gz, self.stats))
        return self.done[name]


GOLDEN_NAMES = ([f"chain:{n}/shuffled" for n in CHAINS] + [f"long:{n}" for n in LONG_RECORDS] + ["wide"] + [c[0] for c in SIMULATED]
                + [f"fuzz:{s}" for s in GOLDEN_FUZZ_SEEDS])


def check_stream(data, gz, stats=None):
    """every member of gz against its 32 KiB of data; returns the members as read"""
    members = read_members(gz)
    assert len(members) == (len(data) + CHUNK - 1) // CHUNK
    assert b"".join(m["out"] for m in members) == data
    off = 0
    for k, m in enumerate(members):
        check_member(m, data[k * CHUNK:(k + 1) * CHUNK], gz[off:off + m["size"]], stats)
        off += m["size"]
    assert off == len(gz)
    return members


def coded_form_fits(body_bits, clen):
    """the kernel's rule, from the numbers of the coded form: the member fits the image, and the blocks are no longer than a stored block of the text"""
    body_bytes = (body_bits + 7) // 8 + 4
    return 10 + 4 + body_bytes + 8 <= IMAGE and body_bytes <= 5 + clen


def check_member(m, chunk, raw, stats=None):
    # ---- round trip ----
    assert m["out"] == chunk
    d = zlib.decompressobj(31)
    assert d.decompress(raw) == chunk and d.eof and d.unused_data == b""        # zlib reads the same bytes from the same member, to its last byte
    assert m["size"] % 4 == 0
    assert m["header"] == b"\x1f\x8b\x08\x08\0\0\0\0\0\xff"                       # deflate, FNAME, mtime 0, XFL 0, OS 255
    assert m["pad"] in (b"", b"x", b"xx", b"xxx")
    blocks = m["blocks"]
    if stats is not None:
        stats["members"] += 1
    # ---- shape ----
    if len(blocks) == 1:
        b = blocks[0]
        assert b["type"] == 0 and b["final"] == 1 and b["len"] == len(chunk)
        # The coded form was longer than 5 + clen or than the image.  Without matches the kernel's coded form is at most: the optimal 15-bit code of
        # the literals, 1 % (the cap on what flattening may cost, below), a header of 74 bits and at most 5 bits for each of 286 + 30 lengths,
        # end of block within the code, the 3 bits of the empty stored block.  If even that fits, the member should have been coded.  (A lower bound:
        # matches, which this cannot see, only make the coded form smaller where they are worth taking.)
        lit = package_merge(literal_histogram(chunk))
        assert not coded_form_fits(lit + lit // 100 + 1 + 74 + 5 * 316 + 3, len(chunk)), ("stored, but literal-only coding fits", len(chunk), lit)
        if stats is not None:
            stats["stored"] += 1
        return
    assert [(b["type"], b["final"]) for b in blocks] == [(2, 0), (0, 1)] and blocks[1]["len"] == 0
    b = blocks[0]
    assert coded_form_fits(b["hdr_bits"] + b["data_bits"] + 3, len(chunk)), ("coded, but the stored form is due", b["hdr_bits"], b["data_bits"], len(chunk))
    # ---- codes ----
    ll, dl, lh, dh = b["ll"], b["dl"], b["lh"], b["dh"]
    assert max(ll) <= 15 and max(dl) <= 15
    assert kraft(ll) == 1 << 15
    n_dist = sum(1 for l in dl if l)
    assert n_dist == 0 or (n_dist == 1 and max(dl) == 1) or kraft(dl) == 1 << 15
    assert b["hclen"] == 19 and b["cl"] == [4] * 13 + [5] * 6
    assert lh[256] == 1
    # the code covers what is coded and nothing else; HLIT / HDIST end at the last used symbol (end-of-block always is one; one distance length is always sent)
    assert [l != 0 for l in ll] == [c != 0 for c in lh[:len(ll)]] and not any(lh[len(ll):])
    assert [l != 0 for l in dl] == [c != 0 for c in dh[:len(dl)]] and not any(dh[len(dl):])
    assert b["hlit"] == max(i for i, c in enumerate(lh) if c) + 1
    assert b["hdist"] == max([i for i, c in enumerate(dh) if c] or [0]) + 1
    # ---- optimality: all optimal codes cost the same, so where 15 bits do not bind the cost IS the heap's ----
    for hist, lens, what in ((lh, ll, "literals / lengths"), (dh, dl, "distances")):
        cost = sum(c * l for c, l in zip(hist, lens))
        best, depth = huffman(hist)
        if depth <= 15:
            assert cost == best, (what, cost, best)
        else:
            pm = package_merge(hist)
            assert pm <= cost and 100 * cost <= 101 * pm, (what, "flattened", cost, pm)
            if stats is not None:
                stats["flattened"] += 1
                stats["worst_excess"] = max(stats["worst_excess"], cost / pm - 1)
    assert b["data_bits"] == sum(c * l for c, l in zip(lh, ll)) + sum(c * l for c, l in zip(dh, dl)) + sum(
        LEN_EXTRA[s - 257] * lh[s] for s in range(257, 286)) + sum(DIST_EXTRA[s] * dh[s] for s in range(30))
    # ---- header (that the decoded lengths are the ones in use: the reader decoded the data with them) ----
    assert b["hdr_bits"] <= header_bits_reference(ll, dl), (b["hdr_bits"], header_bits_reference(ll, dl))
    # ---- tokens ----
    starts = {}
    matches = [t for t in b["tokens"] if not isinstance(t, int)]
    for pos, length, dist in matches:
        assert 3 <= length <= 64 and 1 <= dist <= pos
        assert pos // SPAN == (pos + length - 1) // SPAN, ("a match crosses a span", pos, length)
        starts[pos // SPAN] = starts.get(pos // SPAN, 0) + 1
    assert max(starts.values(), default=0) <= MAX_MATCHES_PER_SPAN
    # 256 spans of at most 8 matches: a member holds at most 2 048 distance symbols.  A distance code deeper than 15 needs chain counts of 17 symbols,
    # 3 570 in all, so the flattening branch of the distance alphabet cannot run (it stays in the kernel: the code construction serves both alphabets).
    assert len(matches) == sum(dh) <= 2048 < 3570 and huffman(dh)[1] <= 15
    if stats is not None:
        stats["matches"] += len(matches)


def check_fuzz(session, seed, n):
    for k, data in enumerate(fuzz_inputs(seed, n)):
        gz = session.ctx.debug_gzip(data)
        try:
            check_stream(data, gz, session.stats)
        except Exception as e:
            raise AssertionError(f"fuzz seed {seed} input {k} ({len(data)} bytes): {e!r}") from e


def check_chains(session):
    """the inputs that need the depth limit: every size in three orders; the unlimited depth is what the recipe promises, the flattened branch is taken,
    and check_member holds the result against package-merge"""
    worst = 0.0
    for n_bytes, depth in CHAINS.items():
        for order in CHAIN_ORDERS:
            data = chain_input(n_bytes, order)
            assert len(data) == n_bytes and huffman(literal_histogram(data))[1] == depth > 15
            _, _, members = session.compress(f"chain:{n_bytes}/{order}")
            b = members[0]["blocks"][0]
            assert len(members) == 1 and b["type"] == 2
            assert huffman(b["lh"])[1] > 15, (n_bytes, order, "the coded histogram does not need the limit")      # check_member took its package-merge branch
            cost = sum(c * l for c, l in zip(b["lh"], b["ll"]))
            worst = max(worst, cost / package_merge(b["lh"]) - 1)
    return worst


def check_long_records(session):
    for rec_len in LONG_RECORDS:
        _, _, members = session.compress(f"long:{rec_len}")
        if rec_len in LONG_REACH:
            found = [t for m in members for b in m["blocks"] if b["type"] == 2 for t in b["tokens"] if not isinstance(t, int) and t[2] == rec_len]
            assert found, ("no match at the distance of one record", rec_len)
            assert DIST_EXTRA[max(s for s in range(30) if DIST_BASE[s] <= rec_len)] >= 12


def check_wide_token(session):
    _, _, members = session.compress("wide")
    b = members[0]["blocks"][0]
    assert b["type"] == 2 and b["max_token_bits"] > 32, ("the generator no longer reaches the split put of pass 3a", b.get("max_token_bits"))
    return b["max_token_bits"]


def name_line_coverage(chunk, tokens, lines_before):
    """of the name-line bytes of a member (lines 0, 4, 8, ... of the stream), the first four lines of the member left out: (bytes, bytes inside matches)"""
    cov = bytearray(len(chunk))
    for t in tokens:
        if not isinstance(t, int):
            cov[t[0]:t[0] + t[1]] = b"\1" * t[1]
    p, k, n_name, n_cov = 0, lines_before, 0, 0
    for ln in chunk.split(b"\n"):
        if k % 4 == 0 and k - lines_before >= 4:
            n_name += len(ln); n_cov += sum(cov[p:p + len(ln)])
        p += len(ln) + 1; k += 1
    return n_name, n_cov


def check_simulated(session, name):
    """matches must earn their place: fewer bits than ANY literal-only block, half of the name lines inside matches, within 10 % of zlib level 1 (the
    design's target: DESIGN.md 6b).  Returns [(coverage, size / zlib level 1)] of the two members."""
    data, gz, members = session.compress(name)
    assert len(members) == 2
    out, off = [], 0
    for k, m in enumerate(members):
        chunk, b = data[k * CHUNK:(k + 1) * CHUNK], m["blocks"][0]
        assert b["type"] == 2
        lit_only, _ = huffman(literal_histogram(chunk))               # a lower bound of every literal-only block, so strictly: no margin
        assert b["data_bits"] < lit_only, (name, k, b["data_bits"], lit_only)
        n_name, n_cov = name_line_coverage(chunk, b["tokens"], data[:k * CHUNK].count(b"\n"))
        assert 2 * n_cov >= n_name > 0, (name, k, "name-line bytes inside matches", n_cov, n_name)
        z1 = len(zlib.compress(chunk, 1))
        assert m["size"] <= 1.10 * z1, (name, k, m["size"], z1)
        out.append((n_cov / n_name, m["size"] / z1))
    return out


def check_determinism(session, names=("sim_150x2", "long:16400", "chain:3569/shuffled", "fuzz:101")):
    """the same text twice through one context, another text of random bytes in between (the device buffers are reused and the kernel loads whole words
    past the text: nothing past the text may reach the output)"""
    rng = random.Random(99)
    for name in names:
        data, gz, _ = session.compress(name)
        noise = bytes(rng.randrange(256) for _ in range(len(data) + 64))
        assert b"".join(m["out"] for m in read_members(session.ctx.debug_gzip(noise))) == noise
        again = session.ctx.debug_gzip(data)
        assert again == gz, (name, "the same text gave other bytes", _first_difference(gz, again))


def _first_difference(a, b):
    return next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))


def golden_digests(session):
    out = {}
    for name in GOLDEN_NAMES:
        data, gz, _ = session.compress(name)
        out[name] = dict(text=len(data), bytes=len(gz), sha256=hashlib.sha256(gz).hexdigest())
    return out


def check_golden(session, names=GOLDEN_NAMES):
    """the members of the named inputs are, byte for byte, the recorded ones (tests/golden/make_gzip_members.py records them from the emulated library):
    a stream that is valid but different is what a race in the histograms or in the rank sort would look like"""
    want = json.load(open(GOLDEN_FILE))["members"]
    assert sorted(want) == sorted(GOLDEN_NAMES)
    for name in names:
        data, gz, _ = session.compress(name)
        got = dict(text=len(data), bytes=len(gz), sha256=hashlib.sha256(gz).hexdigest())
        assert got == want[name], (name, got, want[name], "a valid stream, but not the recorded one")
