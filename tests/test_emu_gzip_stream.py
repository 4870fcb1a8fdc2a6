"""CPU-only: the DEFLATE stream k_gzip makes (dwgsim_amd/csrc/dw_gzip.hip, compiled for the CPU emulation) against the test's own reader and optimal
code costs (tests/gzip_stream.py): code completeness and optimality, the run-length coded header, the shape of a member, what the matches save, the
inputs that need the 15-bit limit, long distances, a match token of more than 32 bits, and the same bytes for the same text -- twice, and as recorded
in tests/golden/gzip_members.json.  tests/test_gpu_gzip_stream.py runs the same checks on the device."""
import os, subprocess, zlib

import pytest

import gzip_stream as G
from dwgsim_amd import api

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def session(golden_dir):
    subprocess.run([os.path.join(HERE, "emu", "build.sh")], check=True, stdout=subprocess.DEVNULL)
    s = G.Session(api.load(os.path.join(HERE, "emu", "libdwgsim_emu.so")), golden_dir)
    yield s
    s.close()


# ---- the reference itself ----
class _Writer:
    def __init__(self):
        self.acc, self.nb = 0, 0

    def put(self, v, n):                  # n bits of v, LSB first (header fields, extra bits)
        self.acc |= v << self.nb; self.nb += n

    def code(self, c, n):                 # a Huffman code: its most significant bit first
        for i in range(n - 1, -1, -1):
            self.put((c >> i) & 1, 1)

    def member(self):
        return b"\x1f\x8b\x08\0\0\0\0\0\0\xff" + self.acc.to_bytes((self.nb + 7) // 8, "little") + bytes(8)


def test_reader_on_streams_zlib_made():
    """the reader against streams of another encoder: the same bytes out of levels 1, 6 and 9 (dynamic blocks, long matches, the whole 32 KiB window),
    of a fixed-code block and of a stored one; a plausible number of tokens"""
    import random
    data = G.fastq_like(random.Random(1), 150000)
    for level in (1, 6, 9):
        c = zlib.compressobj(level, zlib.DEFLATED, 31)
        gz = c.compress(data) + c.flush()
        m = G.read_member(gz)
        assert m["out"] == data and m["size"] == len(gz) and m["pad"] is None
        coded = [b for b in m["blocks"] if b["type"]]
        n_tokens = sum(len(b["tokens"]) for b in coded)
        assert all(3 <= t[1] <= 258 and 1 <= t[2] <= 32768 for b in coded for t in b["tokens"] if not isinstance(t, int))
        assert max(t[2] for b in coded for t in b["tokens"] if not isinstance(t, int)) > 16384
        # every byte is a literal or inside a match, and a token is a byte at least: between the compressed size in bytes / 6 (48 bits) and the text
        assert len(gz) // 6 < n_tokens < len(data)
        assert all(sum(b["lh"]) == len(b["tokens"]) + 1 for b in coded)
        assert sum(1 if isinstance(t, int) else t[1] for b in coded for t in b["tokens"]) + sum(b["len"] for b in m["blocks"] if not b["type"]) == len(data)
    for level, typ in ((0, 0), (6, 1)):
        c = zlib.compressobj(level, zlib.DEFLATED, 31)
        gz = c.compress(b"abcabcabc\n") + c.flush()
        m = G.read_member(gz)
        assert m["out"] == b"abcabcabc\n" and [b["type"] for b in m["blocks"]] == [typ]
    assert [m["out"] for m in G.read_members(gz + gz)] == [b"abcabcabc\n"] * 2


def test_reader_rejects_what_zlib_rejects():
    bad = {}
    w = _Writer(); w.put(1, 1); w.put(0, 2); w.put(0, 5); w.put(3, 16); w.put(0xFFFF ^ 2, 16); w.put(0x414141, 24)
    bad["LEN and NLEN"] = w.member()
    w = _Writer(); w.put(1, 1); w.put(1, 2); w.code(0x30 + 65, 8); w.code(1, 7); w.code(1, 5); w.code(0, 7)      # 'A', then length 3 at distance 2
    bad["a distance before the start"] = w.member()
    w = _Writer(); w.put(1, 1); w.put(2, 2); w.put(0, 5); w.put(0, 5); w.put(0, 4)
    for l in (1, 1, 1, 0):
        w.put(l, 3)                       # three code-length codes of one bit
    w.put(0, 64)
    bad["over-subscribed"] = w.member()
    w = _Writer(); w.put(1, 1); w.put(2, 2); w.put(0, 5); w.put(0, 5); w.put(0, 4)
    for l in (2, 2, 0, 0):
        w.put(l, 3)                       # two code-length codes of two bits
    w.put(0, 64)
    bad["incomplete"] = w.member()
    w = _Writer(); w.put(1, 1); w.put(3, 2); w.put(0, 32)
    bad["block type 3"] = w.member()
    for what, gz in bad.items():
        with pytest.raises(zlib.error):
            zlib.decompressobj(31).decompress(gz)
        with pytest.raises(G.StreamError, match=what):
            G.read_member(gz)
    # ... and reads what zlib reads: the same block with the distance in reach, a damaged CRC, a damaged length
    w = _Writer(); w.put(1, 1); w.put(1, 2); w.code(0x30 + 65, 8); w.code(1, 7); w.code(0, 5); w.code(0, 7)      # 'A', then length 3 at distance 1
    gz = bytearray(w.member())
    gz[-8:] = zlib.crc32(b"AAAA").to_bytes(4, "little") + (4).to_bytes(4, "little")
    assert G.read_member(bytes(gz))["out"] == b"AAAA" == zlib.decompress(bytes(gz), 31)
    assert G.read_member(bytes(gz))["blocks"][0]["tokens"] == [65, (1, 3, 1)]
    for at, what in ((-8, "CRC"), (-4, "ISIZE")):
        g2 = bytearray(gz); g2[at] ^= 1
        with pytest.raises(G.StreamError, match=what):
            G.read_member(bytes(g2))
        with pytest.raises(zlib.error):
            zlib.decompress(bytes(g2), 31)


def test_optimal_costs_and_the_header_count():
    """the heap against package-merge where no limit binds, package-merge against exhaustive search on small histograms, the chain recipe, and
    the header count on cases worked by hand"""
    import itertools, random
    rng = random.Random(3)
    for _ in range(200):
        h = [rng.choice([0, 1, 2, 3, 50, 1000, rng.randrange(1, 40000)]) for _ in range(rng.randrange(2, 40))]
        if sum(1 for x in h if x) < 2:
            continue
        cost, depth = G.huffman(h)
        assert G.package_merge(h, 15) == cost if depth <= 15 else G.package_merge(h, 15) > cost
        assert G.package_merge(h, max(depth, 1)) == cost
    for h in ([1, 1, 2, 4, 8, 16], [1, 1, 1, 3, 4, 7, 11], [5, 5, 5, 5, 5], [1, 2, 3, 4, 5, 6, 7]):
        for limit in (3, 4, 5):
            best = min(sum(c * l for c, l in zip(h, ls)) for ls in itertools.product(range(1, limit + 1), repeat=len(h))
                       if sum(1 << (limit - l) for l in ls) <= 1 << limit)
            assert G.package_merge(h, limit) == best, (h, limit)
    for n in range(2, 24):
        assert G.huffman([1] + G.chain_weights(n))[1] == n
    assert [(sum(G.chain_weights(d)), d) for d in (16, 17, 19, 20)] == list(G.CHAINS.items()) and sum(G.chain_weights(15)) < 3569
    fixed = 3 + 5 + 5 + 4 + 57
    assert G.header_bits_reference([8], [0]) == fixed + 4 + 4
    assert G.header_bits_reference([8] * 7, [0]) == fixed + 4 + (5 + 2) + 4                         # 8, then six more by one symbol 16
    assert G.header_bits_reference([8] * 9, [0]) == fixed + 4 + (5 + 2) + 2 * 4 + 4                 # ... two left over: written out
    assert G.header_bits_reference([13] * 4, [5, 5]) == fixed + 5 + (5 + 2) + 4 + 4
    assert G.header_bits_reference([0] * 2 + [3], [0] * 10) == fixed + 2 * 4 + 4 + (5 + 3)          # zeros: two written out; ten by one symbol 17
    assert G.header_bits_reference([0] * 150 + [3], [1]) == fixed + (5 + 7) + (5 + 7) + 4 + 4       # 138 and 12 by symbol 18


# ---- the kernel ----
@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_fuzzed_fastq_like_text_on_cpu_emulation(session, seed):
    G.check_fuzz(session, seed, 60)


def test_chain_histograms_take_the_depth_limit_on_cpu_emulation(session):
    worst = G.check_chains(session)
    print(f"\nflattened codes: at most {worst:.3%} over the package-merge optimum (cap 1 %)")


def test_long_records_reach_distances_of_13_extra_bits_on_cpu_emulation(session):
    G.check_long_records(session)


def test_a_match_token_of_more_than_32_bits_on_cpu_emulation(session):
    assert G.check_wide_token(session) == 33


@pytest.mark.parametrize("name", [c[0] for c in G.SIMULATED])
def test_matches_earn_their_place_on_simulated_text_on_cpu_emulation(session, name):
    got = G.check_simulated(session, name)
    print("\n" + name + ": " + "; ".join(f"name-line bytes inside matches {c:.2f}, member / zlib level 1 {z:.3f}" for c, z in got))


def test_the_same_text_gives_the_same_bytes_on_cpu_emulation(session):
    G.check_determinism(session)


def test_members_are_the_recorded_ones_on_cpu_emulation(session):
    G.check_golden(session)
