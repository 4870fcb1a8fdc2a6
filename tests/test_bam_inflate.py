"""The inflater and the BGZF framing of dwgsim_eval-hip's BAM input (dwgsim_amd/csrc/dw_inflate.hpp, dw_bam.hpp) in a stand-alone program
(tests/bam_inflate_main.cpp) built with -fsanitize=address,undefined: valid streams of every zlib level and strategy must come out byte for
byte with the right CRC-32, and damaged ones must return without a sanitizer report and without a byte written past dst_cap."""
import os, random, struct, subprocess, zlib
import pytest

import bam_io as B
import eval_sam as S

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "dwgsim_amd", "csrc")
LEVELS = [0, 1, 6, 9]
STRATEGIES = [zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE]


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("inflate") / "bam_inflate_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(HERE, "bam_inflate_main.cpp"), "-o", exe], check=True)
    return exe


def sam_like(rng, n):
    contigs = [("chr1", 5000), ("chr10", 3000)]
    return b"".join(r + b"\n" for r in S.records(rng, S.synth_names(rng, contigs, n), contigs))


def inputs():
    rng = random.Random(7)
    return {"empty": b"", "one": b"x", "zeros": bytes(65280), "random": rng.randbytes(65280), "sam": sam_like(rng, 150)[:65280]}


def deflate(data, level, strategy, pieces=None):
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    if pieces:
        step = max(1, len(data) // pieces)
        return b"".join(co.compress(data[i:i + step]) + co.flush(zlib.Z_FULL_FLUSH if (i // step) % 2 else zlib.Z_SYNC_FLUSH)
                        for i in range(0, step * pieces, step)) + co.compress(data[step * pieces:]) + co.flush()
    return co.compress(data) + co.flush()


def case(kind, src, dst_cap, expected):
    return struct.pack("<BIIII", kind, len(src), dst_cap, len(expected), zlib.crc32(expected)) + src + expected


def run(prog, tmp_path, cases):
    path = tmp_path / "cases.bin"
    path.write_bytes(b"".join(cases))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([prog, str(path)], capture_output=True, env=env, timeout=300)
    assert p.returncode == 0 and p.stderr == b"", p.stderr.decode(errors="replace")[-3000:]
    return dict((l.split()[0], [int(x) for x in l.split()[1::2]]) for l in p.stdout.decode().splitlines())


def test_valid_streams(prog, tmp_path):
    cases = []
    for name, data in inputs().items():
        for level in LEVELS:
            for strategy in STRATEGIES:
                z = deflate(data, level, strategy)
                assert zlib.decompress(z, -15) == data
                cases.append(case(0, z, len(data), data))
                if 18 + len(z) + 8 <= 65536:
                    cases.append(case(1, B.bgzf_block(data, level, strategy), len(data), data))
    rng = random.Random(1)
    many = sam_like(rng, 300)
    for level in LEVELS[1:]:
        z = deflate(many, level, zlib.Z_DEFAULT_STRATEGY, pieces=40)
        assert zlib.decompress(z, -15) == many
        cases.append(case(0, z, len(many), many))
    cases.append(case(1, B.EOF_BLOCK, 0, b""))
    out = run(prog, tmp_path, cases)
    assert out["raw"] == [5 * 16 + 3] and out["bgzf"][0] >= 4 * 16 + 1


def test_damaged_streams(prog, tmp_path):
    rng = random.Random(2024)
    text = sam_like(rng, 120)
    bases = [(B.bgzf_block(d, level, strategy), d) for d in (text[:20000], bytes(3000) + text[:500], rng.randbytes(2000))
             for level, strategy in ((6, zlib.Z_DEFAULT_STRATEGY), (1, zlib.Z_FIXED), (9, zlib.Z_RLE), (0, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_HUFFMAN_ONLY))]
    cases, n_cut = [], 0
    for k in range(2000):
        block, data = bases[k % len(bases)]
        b = bytearray(block)
        if rng.random() < 0.3:
            b = b[:rng.randrange(len(b))]; n_cut += 1
        else:
            for _ in range(rng.randrange(1, 4)):
                # most flips go into the deflate stream, some into the header and the trailer
                at = rng.randrange(18, len(b) - 8) if rng.random() < 0.85 else rng.randrange(len(b))
                b[at] ^= 1 << rng.randrange(8)
        cases.append(case(2, bytes(b), len(data), data))
    out = run(prog, tmp_path, cases)
    damaged, refused, undetected = out["damaged"]
    # a flipped bit that changes neither the data nor ISIZE nor the CRC-32 (MTIME, the padding bits behind the last code) passes; damage that
    # changes the data must be refused, and so must every cut block
    assert damaged == 2000 and undetected == 0 and refused >= n_cut > 400
