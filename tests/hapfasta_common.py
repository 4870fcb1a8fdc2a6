"""The haplotype FASTA (include/dwgsim_hip.h dwgsim_hip_haplotype_fasta; DESIGN.md "6d"): a plain-Python model of the text and the cases
tests/test_emu_hapfasta.py (CPU emulation) and tests/test_gpu_hapfasta.py (device) both run.  Every check_* function takes the loaded library.

The model: a haplotype is the reference, normalised (upper case; everything but A, C, G, T is N), with a list of edits applied --
(pos, kind, bases, mask): pos = 0-based cell, kind 'S' (the cell's base becomes bases), 'D' (the cell emits nothing), 'I' (bases follow the cell's
own base), mask = 1 (haplotype 1), 2 (haplotype 2) or 3 (both).  A cell carries one edit per haplotype."""
import gzip
import os
import subprocess

import numpy as np

from dwgsim_amd import api

WIDTHS = (60, 1, 7, 0)
LAYOUT_LENGTHS = (1, 59, 60, 61, 120, 4095, 4096, 4097, 8193)      # line ends, block ends (4096 cells), more than one block
# seventeen contigs, names of 1 ... 17 characters (header lines of 3 ... 19 bytes: a record body starts at every offset modulo 16); the lengths above and a few more
LAYOUT_17 = LAYOUT_LENGTHS + (2, 16, 17, 119, 121, 4094, 8192, 33)
IUPAC = "XACMGRSVTWYHKDBN"      # indexed by the set of bases, A = 1, C = 2, G = 4, T = 8
PIECE_MAX = 32 << 20            # the job level hands the text over in pieces of at most this size


def synth(seed: int, n: int) -> np.ndarray:
    """random ACGT with a few runs of N and some lower-case letters, as the bytes of a FASTA sequence"""
    rng = np.random.default_rng(seed)
    a = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].copy()
    if n >= 200:
        for _ in range(3):
            s = int(rng.integers(0, n - 20)); a[s:s + int(rng.integers(1, 20))] = ord("N")
        for _ in range(3):
            s = int(rng.integers(0, n - 40)); a[s:s + 40] |= 0x20
    return a


def normalise(arr) -> str:
    s = (arr if isinstance(arr, (bytes, bytearray)) else np.asarray(arr, dtype=np.uint8).tobytes()).decode("latin-1").upper()
    return "".join(c if c in "ACGT" else "N" for c in s)


def wrap(name: str, seq: str, width: int) -> bytes:
    """one record: '>' name, then the bases in lines of `width` (0: one line), every line ended by a newline; no bases: the header alone"""
    out = [">" + name + "\n"]
    if seq:
        if width == 0:
            out.append(seq + "\n")
        else:
            out.extend(seq[i:i + width] + "\n" for i in range(0, len(seq), width))
    return "".join(out).encode()


def apply_edits(reference: str, edits, hap: int) -> str:
    mine = {}
    for pos, kind, bases, mask in edits:
        if mask & (1 << hap):
            assert pos not in mine, "a cell carries one edit per haplotype"
            mine[pos] = (kind, bases)
    out = []
    for i, c in enumerate(reference):
        kind, bases = mine.get(i, ("", ""))
        if kind == "D":
            continue
        out.append(bases if kind == "S" else c)
        if kind == "I":
            out.append(bases)
    return "".join(out)


def edits_to_txt(name: str, reference: str, edits) -> str:
    """the edits as lines of a mutations.txt (-m): 1-based position, reference base or '-', new base (IUPAC code of both for one haplotype) / '-' / inserted bases, haplotype mask"""
    lines = []
    for pos, kind, bases, mask in sorted(edits):
        r = reference[pos]
        if kind == "S":
            alt = bases if mask == 3 else IUPAC[(1 << "ACGT".index(r)) | (1 << "ACGT".index(bases))]
            lines.append(f"{name}\t{pos + 1}\t{r}\t{alt}\t{mask}\n")
        elif kind == "D":
            lines.append(f"{name}\t{pos + 1}\t{r}\t-\t{mask}\n")
        else:
            lines.append(f"{name}\t{pos + 1}\t-\t{bases}\t{mask}\n")
    return "".join(lines)


def parse_mutations_txt(txt: bytes) -> dict:
    """a job's mutations.txt -> {contig: edits}.  A heterozygous substitution's base is the IUPAC code minus the reference base."""
    out = {}
    for line in txt.decode().splitlines():
        name, pos, ref, alt, mask = line.split("\t")
        pos, mask = int(pos) - 1, int(mask)
        if ref == "-":
            e = (pos, "I", alt, mask)
        elif alt == "-":
            e = (pos, "D", "", mask)
        elif mask == 3:
            e = (pos, "S", alt, mask)
        else:
            left = IUPAC.index(alt) & ~(1 << "ACGT".index(ref))
            e = (pos, "S", "ACGT"[left.bit_length() - 1], mask)
        out.setdefault(name, []).append(e)
    return out


def revcomp(s: str) -> str:
    return s[::-1].translate(str.maketrans("ACGTN", "TGCAN"))


def records(text: bytes) -> dict:
    """a FASTA text -> {name: sequence}"""
    out = {}
    for rec in text.decode().split(">")[1:]:
        head, _, body = rec.partition("\n")
        out[head] = body.replace("\n", "")
    return out


def expected(contigs, width: int, edits=None, hap: int = 0) -> bytes:
    return b"".join(wrap(n, apply_edits(normalise(a), (edits or {}).get(n, []), hap), width) for n, a in contigs)


def layout_contigs():
    return [(chr(97 + k) * (k + 1), synth(100 + k, n)) for k, n in enumerate(LAYOUT_17)]


# ---- 1. unmutated: layout only ----
def check_layout(lib):
    contigs = layout_contigs()
    assert sorted(len(n) for n, _ in contigs) == list(range(1, 18)) and set(LAYOUT_LENGTHS) <= {len(a) for _, a in contigs}
    p = api.parse_flags("-z 3 -r 0 -M 2", lib)
    with api.Context(p, 0, lib) as ctx:
        h0 = ctx.add_contigs(contigs)
        ctx.mutate(h0)
        for w in WIDTHS:
            want = expected(contigs, w)
            for hap in (0, 1):
                got = ctx.haplotype_fasta(h0, hap, w)
                assert got == want, (w, hap)
                assert ctx.haplotype_fasta(h0, hap, w) == want, "the same call twice"
                for k, (name, arr) in enumerate(contigs):      # where each record lies
                    off, nbytes, bases = ctx.haplotype_layout(h0 + k, hap)
                    assert want[off:off + nbytes] == wrap(name, normalise(arr), w) and bases == len(arr), (w, hap, name)
        ctx.drop_contig(h0)
    for w in WIDTHS:      # a group each (a record body then starts 3 ... 19 bytes into its text: every offset modulo 16), and all in one group
        want = expected(contigs, w)
        each = api.run_job(api.parse_flags("-z 3 -r 0 -M 2", lib), contigs, lib=lib, group_bp=0, haplotypes=True, hap_width=w)
        one = api.run_job(api.parse_flags("-z 3 -r 0 -M 2", lib), contigs, lib=lib, group_bp=1 << 30, haplotypes=True, hap_width=w)
        assert each.haplotypes == {0: want, 1: want} and one.haplotypes == {0: want, 1: want}, w


# ---- 2. placed edits through a -m file ----
def placed_case():
    """Two contigs in one group, cB behind cA, so that nothing of the padding between them may leak.  The file-driven walk left-justifies what the file
    places, as the reference does (mut.c:427-589): an insertion moves left while its last base equals the base in front of its cell, a deletion run
    while the base in front of it equals the run's last base.  The edits below are placed where neither holds -- the bases next to them are pinned --
    so that the cells are the edits as written.  (No edit had to move to a position other than the ones the issue names: substitutions and
    deletions on the cells named, insertions behind them.)"""
    a, b = synth(7, 9000), synth(8, 5000)
    pins_a = {0: "A", 8999: "G", 8998: "A", 4094: "A", 4095: "C", 4096: "G", 999: "A", 1000: "C", 1999: "A", 2004: "C", 2999: "A", 3000: "T"}
    pins_a.update({q: "ACGT"[q & 3] for q in range(2000, 2004)})
    pins_b = {0: "C", 4999: "T", 4089: "A", 4100: "C"}
    pins_b.update({q: "ACGT"[q & 3] for q in range(4090, 4100)})
    long_ins = [100, 300, 500, 700, 900, 1100]      # six insertions of 1000 bases in cB's first block: it emits 10 096 bases, more than one staging window of the write pass
    pins_b.update({q - 1: "A" for q in long_ins}); pins_b.update({q: "C" for q in long_ins})
    for arr, pins in ((a, pins_a), (b, pins_b)):
        for q, ch in pins.items():
            arr[q] = ord(ch)
    big = "".join("ACGT"[(7 * q + q // 5) & 3] for q in range(199)) + "C"      # 200 inserted bases behind cell 1000 (base in front of the cell: A; last inserted base: C)
    edits = {
        "cA": [(0, "S", "T", 3),                       # a substitution at the first base
               (8999, "I", "TTC", 3),                  # an insertion behind the last base of the contig (base in front: A)
               (4095, "I", "GGT", 1),                  # insertions at a block's last cell (haplotype 1 only) ...
               (4096, "I", "TA", 3),                   # ... and at the next block's first cell
               (1000, "I", big, 3),
               (3000, "I", "CCCCCCG", 2)]              # heterozygous indels: the two haplotypes differ in length
              + [(q, "D", "", 1) for q in range(2000, 2005)],
        "cB": [(0, "S", "G", 2),                       # haplotype 2 only
               (4999, "S", "A", 3)]                    # a substitution at the last base
              + [(q, "D", "", 3) for q in range(4090, 4101)]       # a homozygous deletion across a block boundary (cells 4090 ... 4100)
              + [(q, "I", "".join("ACGT"[(3 * t + t // 7 + q) & 3] for t in range(999)) + "G", 3) for q in long_ins],
    }
    return [("cA", a), ("cB", b)], edits


def check_placed_edits(lib, tmp_path):
    contigs, edits = placed_case()
    path = os.path.join(str(tmp_path), "placed.txt")
    with open(path, "w") as f:
        for name, arr in contigs:
            f.write(edits_to_txt(name, normalise(arr), edits[name]))
    for w in (60, 7, 0):
        p = api.parse_flags(f"-z 5 -M 2 -m {path}", lib)
        res = api.run_job(p, contigs, lib=lib, group_bp=1 << 30, haplotypes=True, hap_width=w)
        for hap in (0, 1):
            assert res.haplotypes[hap] == expected(contigs, w, edits, hap), (w, hap)
        h = [records(res.haplotypes[q]) for q in (0, 1)]
        assert len(h[0]["cA"]) == 9000 + 3 + 3 + 2 + 200 - 5 and len(h[1]["cA"]) == 9000 + 3 + 2 + 200 + 7 and len(h[0]["cB"]) == len(h[1]["cB"]) == 5000 - 11 + 6000


# ---- 3. a random walk against the job's own mutations.txt ----
RANDOM_WALKS = ("-z 11 -r 0.02 -R 0 -N 200 -1 50 -2 50", "-z 12 -r 0.02 -R 1 -X 0.5 -N 200 -1 50 -2 50")      # substitutions only; indels only (SURVEY "Hom-deletion left-shift": mixed edits are left to check_reads)


def check_random_walk(lib, flags):
    contigs = [("walk", synth(21, 20000))]
    res = api.run_job(api.parse_flags(flags, lib), contigs, lib=lib, haplotypes=True, hap_width=60)
    edits = parse_mutations_txt(res.mutations_txt)
    assert len(edits["walk"]) > 200
    for hap in (0, 1):
        assert res.haplotypes[hap] == expected(contigs, 60, edits, hap), hap
    assert res.haplotypes[0] != res.haplotypes[1]


# ---- 4. the reads come from the written genomes ----
def check_reads(lib, haploid: bool):
    contigs = [("chrA", synth(31, 10000)), ("chrB", synth(32, 9500))]
    flags = "-e 0 -E 0 -y 0 -r 0.02 -R 0.3 -X 0.5 -N 2000 -1 70 -2 70 -z 17" + (" -H" if haploid else "")
    res = api.run_job(api.parse_flags(flags, lib), contigs, lib=lib, group_bp=1 << 30, haplotypes=True, hap_width=0)
    hap = [records(res.haplotypes[q]) for q in (0, 1)]
    if haploid:
        assert res.haplotypes[0] == res.haplotypes[1]
    else:
        assert res.haplotypes[0] != res.haplotypes[1]
    n = 0
    for s in (api.STREAM_BWA1, api.STREAM_BWA2):
        lines = res.streams[s].decode().split("\n")
        for name, seq in zip(lines[0::4], lines[1::4]):
            if not name:
                continue
            contig = name[1:name.index("_")]
            rc = revcomp(seq)
            assert any(seq in hap[q][contig] or rc in hap[q][contig] for q in (0, 1)), name
            n += 1
    assert n == 4000


# ---- 5. the job level against the context level ----
def levels_case(tmp_path):
    """five contigs; `allN` is passed over (-x, skip #1) and `tiny` too (skip #3: shorter than the insert size): neither has a record"""
    contigs = [("g1", synth(41, 6000)), ("allN", np.full(3000, ord("N"), dtype=np.uint8)), ("g2", synth(42, 9000)), ("tiny", synth(43, 100)), ("g3", synth(44, 5000))]
    bed = os.path.join(str(tmp_path), "all.bed")
    with open(bed, "w") as f:
        for name, arr in contigs:
            f.write(f"{name}\t0\t{len(arr)}\n")
    return contigs, f"-z 23 -r 0.01 -R 0.2 -N 600 -1 60 -2 60 -x {bed}"


def check_levels(lib, tmp_path):
    contigs, flags = levels_case(tmp_path)
    ctx_level = api.run_job(api.parse_flags(flags, lib), contigs, lib=lib, group_bp=0, haplotypes=True, hap_width=60)
    job_level = api.run_job_api(api.parse_flags(flags, lib), contigs, devices=[0], gzip_on_gpu=False, batch_pairs=150, group_bp=8000, lib=lib, haplotypes=True, hap_width=60)
    for hap in (0, 1):
        assert list(records(ctx_level.haplotypes[hap])) == ["g1", "g2", "g3"]
        assert job_level.haplotypes[hap] == ctx_level.haplotypes[hap], hap      # (the pieces of a haplotype, in the order they arrived)
    assert job_level.haplotype_pieces and all(0 < n <= PIECE_MAX for _, n in job_level.haplotype_pieces)
    assert job_level.mutations_txt == ctx_level.mutations_txt and job_level.streams == ctx_level.streams
    plain = api.run_job_api(api.parse_flags(flags, lib), contigs, devices=[0], gzip_on_gpu=False, batch_pairs=150, group_bp=8000, lib=lib)
    assert plain.haplotypes == {} and plain.streams == job_level.streams and plain.mutations_txt == job_level.mutations_txt
    # -M changes which files are written (and, without reads, no contig is passed over), not what a contig's haplotypes are
    mut_only = api.run_job(api.parse_flags(flags + " -M 2", lib), contigs, lib=lib, group_bp=0, haplotypes=True, hap_width=60)
    for hap in (0, 1):
        got, want = records(mut_only.haplotypes[hap]), records(ctx_level.haplotypes[hap])
        assert list(got) == [n for n, _ in contigs] and all(got[n] == want[n] for n in want), hap


# ---- 6. the command line ----
def check_cli(lib, cli, tmp_path, gzip_mode):
    contigs, flags = levels_case(tmp_path)
    fa = os.path.join(str(tmp_path), "in.fa")
    with open(fa, "w") as f:
        for name, arr in contigs:
            s = bytes(bytearray(arr)).decode()
            f.write(f">{name}\n" + "".join(s[i:i + 70] + "\n" for i in range(0, len(s), 70)))
    assert [(n, bytes(bytearray(a))) for n, a in api.read_fasta(fa)] == [(n, bytes(bytearray(a))) for n, a in contigs]
    base = {k: v for k, v in os.environ.items() if not k.startswith("DWGSIM_HIP_HAPLOTYPES")}
    base.update(DWGSIM_HIP_GZIP=gzip_mode, DWGSIM_HIP_GROUP_BP="8000", DWGSIM_HIP_BATCH="150")
    outs = {}
    for tag, extra in (("w80", {"DWGSIM_HIP_HAPLOTYPES": "1", "DWGSIM_HIP_HAPLOTYPES_WIDTH": "80"}), ("w0", {"DWGSIM_HIP_HAPLOTYPES": "yes", "DWGSIM_HIP_HAPLOTYPES_WIDTH": "0"}),
                       ("off", {}), ("zero", {"DWGSIM_HIP_HAPLOTYPES": "0"})):
        prefix = os.path.join(str(tmp_path), tag)
        subprocess.run([cli] + flags.split() + [fa, prefix], check=True, stderr=subprocess.DEVNULL, env=dict(base, **extra), timeout=600)
        outs[tag] = {}
        for name in sorted(os.listdir(str(tmp_path))):
            if name.startswith(tag + "."):
                data = open(os.path.join(str(tmp_path), name), "rb").read()
                outs[tag][name[len(tag):]] = gzip.decompress(data) if name.endswith(".gz") else data      # (the FASTQ files by their text)
    for tag, w in (("w80", 80), ("w0", 0)):
        want = api.run_job(api.parse_flags(flags, lib), contigs, lib=lib, group_bp=0, fetch=False, haplotypes=True, hap_width=w).haplotypes
        assert outs[tag][".hap1.fa"] == want[0] and outs[tag][".hap2.fa"] == want[1], tag
    others = {k: v for k, v in outs["off"].items()}
    assert ".hap1.fa" not in others and ".hap2.fa" not in others and len(others) == 5
    assert outs["zero"] == others
    for tag in ("w80", "w0"):      # every existing output is what it is without the variable
        assert {k: v for k, v in outs[tag].items() if not k.startswith(".hap")} == others, tag


# ---- 7. argument and state errors ----
def check_errors(lib):
    import ctypes as C
    p = api.parse_flags("-z 3 -r 0.01 -M 2", lib)
    with api.Context(p, 0, lib) as ctx:
        h = ctx.add_contigs([("e", synth(51, 5000))])
        n = C.c_uint64(0)
        assert lib.dwgsim_hip_haplotype_fasta(ctx.h, h, 0, 60, C.byref(n)) == -6      # DWGSIM_HIP_ERR_STATE: before the walk
        said = lib.dwgsim_hip_last_error(ctx.h)
        assert lib.dwgsim_hip_mutations_text(ctx.h, h, None, None, None, None) == -6 and lib.dwgsim_hip_last_error(ctx.h) == said
        assert lib.dwgsim_hip_haplotype_layout(ctx.h, h, 0, None, None, None) == -6
        buf = C.create_string_buffer(16)
        assert lib.dwgsim_hip_haplotype_fetch(ctx.h, 0, 0, buf, 1) == -6
        ctx.mutate(h)
        assert lib.dwgsim_hip_haplotype_fasta(ctx.h, h, 2, 60, C.byref(n)) == -1       # DWGSIM_HIP_ERR_ARG
        assert lib.dwgsim_hip_haplotype_fasta(ctx.h, h, -1, 60, C.byref(n)) == -1
        assert lib.dwgsim_hip_haplotype_fasta(ctx.h, h, 0, -1, C.byref(n)) == -1
        assert lib.dwgsim_hip_haplotype_fasta(ctx.h, h + 1, 0, 60, C.byref(n)) == -1   # no such contig
        assert lib.dwgsim_hip_haplotype_fasta(ctx.h, h, 0, 60, C.byref(n)) == 0 and n.value > 5000
        assert lib.dwgsim_hip_haplotype_fetch(ctx.h, 0, n.value - 8, buf, 8) == 0 and buf.raw[7:8] == b"\n"
        assert lib.dwgsim_hip_haplotype_fetch(ctx.h, 0, n.value - 8, buf, 9) == -1      # past the end
        assert lib.dwgsim_hip_haplotype_fetch(ctx.h, 0, n.value + 1, buf, 0) == -1
        assert lib.dwgsim_hip_haplotype_fetch(ctx.h, 0, n.value, buf, 0) == 0
        assert lib.dwgsim_hip_haplotype_fetch(ctx.h, 2, 0, buf, 1) == -1
        assert lib.dwgsim_hip_haplotype_fetch(ctx.h, 1, 0, buf, 1) == -6                # haplotype 2 has not been built
        ctx.mutate(h)                                                                   # walked again: the text is gone
        assert lib.dwgsim_hip_haplotype_fetch(ctx.h, 0, 0, buf, 1) == -6
