"""The chain files (include/dwgsim_hip.h dwgsim_hip_haplotype_chain / dwgsim_hip_chain_format; DESIGN.md "6g"): a plain-Python model of the blocks and the
text, and the cases tests/test_emu_chain.py (CPU emulation) and tests/test_gpu_chain.py (device) both run.  Every check_* function takes the loaded library.

The model works on the edit model of tests/hapfasta_common.py -- (pos, kind, bases, mask) per contig.  A cell is aligned unless it is deleted; an
ungapped block is a maximal run of consecutive aligned cells in which no cell but the last has inserted bases behind it.  Blocks are (size, d_ref, d_hap):
the deleted cells and inserted bases between a block and the next one -- for the last block, what lies behind it (not part of the chain's text)."""
import gzip
import os
import subprocess

import numpy as np

import hapfasta_common as H
from dwgsim_amd import api

DIRECTIONS = ("to_ref", "from_ref")
KEYS = [(hap, d) for hap in (0, 1) for d in DIRECTIONS]
FILES = {(0, "to_ref"): ".hap1.to_ref.chain", (0, "from_ref"): ".hap1.from_ref.chain", (1, "to_ref"): ".hap2.to_ref.chain", (1, "from_ref"): ".hap2.from_ref.chain"}


# ---- the model ----
def chain_blocks(l: int, edits, hap: int):
    """(ref_start, [(size, d_ref, d_hap), ...]) of haplotype `hap` of a contig of l cells; no aligned cell: (0, [])"""
    deleted, inserted = set(), {}
    for pos, kind, bases, mask in edits:
        if mask & (1 << hap):
            if kind == "D":
                deleted.add(pos)
            elif kind == "I" and bases:
                inserted[pos] = len(bases)
    runs = []      # [first cell, last cell]
    for i in range(l):
        if i in deleted:
            continue
        if runs and runs[-1][1] == i - 1 and (i - 1) not in inserted:
            runs[-1][1] = i
        else:
            runs.append([i, i])
    if not runs:
        return 0, []
    blocks = []
    for k, (s, e) in enumerate(runs):
        nxt = runs[k + 1][0] if k + 1 < len(runs) else l
        blocks.append((e - s + 1, nxt - e - 1, inserted.get(e, 0)))
    return runs[0][0], blocks


def format_chain(name: str, l: int, ref_start: int, blocks, direction: str, chain_id: int) -> bytes:
    score = sum(b[0] for b in blocks)
    hap_len = sum(b[0] + b[2] for b in blocks)
    ref = f"{name} {l} + {ref_start} {l - blocks[-1][1]}"
    hap = f"{name} {hap_len} + 0 {hap_len - blocks[-1][2]}"
    out = [f"chain {score} {ref} {hap} {chain_id}\n" if direction == "from_ref" else f"chain {score} {hap} {ref} {chain_id}\n"]
    for size, d_ref, d_hap in blocks[:-1]:
        out.append(f"{size}\t{d_ref}\t{d_hap}\n" if direction == "from_ref" else f"{size}\t{d_hap}\t{d_ref}\n")
    out.append(f"{blocks[-1][0]}\n\n")
    return "".join(out).encode()


def expected(contigs, edits=None) -> dict:
    """the four files of a job over `contigs` (the simulated ones, FASTA order): a haplotype without an aligned cell has no chain and takes no id"""
    out = {}
    for hap in (0, 1):
        made = []
        for name, arr in contigs:
            r0, blocks = chain_blocks(len(arr), (edits or {}).get(name, []), hap)
            if blocks:
                made.append((name, len(arr), r0, blocks))
        for d in DIRECTIONS:
            out[(hap, d)] = b"".join(format_chain(n, l, r0, b, d, k + 1) for k, (n, l, r0, b) in enumerate(made))
    return out


def parse_chains(text: bytes):
    """a chain file -> [{score, t: (name, size, strand, start, end), q: (...), id, blocks: [(size, dt, dq)], last}] (a parser of the tests' own)"""
    out = []
    lines = text.decode().split("\n")
    assert lines[-1] == "", "the file ends with a newline"
    k = 0
    while k < len(lines) - 1:
        f = lines[k].split(" ")
        assert f[0] == "chain" and len(f) == 13, lines[k]
        side = lambda q: (f[q], int(f[q + 1]), f[q + 2], int(f[q + 3]), int(f[q + 4]))
        c = {"score": int(f[1]), "t": side(2), "q": side(7), "id": int(f[12]), "blocks": []}
        k += 1
        while True:
            g = lines[k].split("\t")
            k += 1
            if len(g) == 1:
                c["last"] = int(g[0])
                break
            assert len(g) == 3, lines[k - 1]
            c["blocks"].append(tuple(int(x) for x in g))
        assert lines[k] == "", "an empty line ends a chain"
        k += 1
        sizes = [b[0] for b in c["blocks"]] + [c["last"]]
        assert c["score"] == sum(sizes) and all(s > 0 for s in sizes) and all(b[1] > 0 or b[2] > 0 for b in c["blocks"])
        for _, size, strand, start, end in (c["t"], c["q"]):
            assert strand == "+" and 0 <= start < end <= size
        assert c["t"][4] - c["t"][3] == sum(sizes) + sum(b[1] for b in c["blocks"]) and c["q"][4] - c["q"][3] == sum(sizes) + sum(b[2] for b in c["blocks"])
        out.append(c)
    return out


def flipped(chains):
    return [dict(c, t=c["q"], q=c["t"], blocks=[(s, dq, dt) for s, dt, dq in c["blocks"]]) for c in chains]


def check_directions(chain: dict):
    """every to_ref file is its from_ref file with target and query exchanged"""
    for hap in (0, 1):
        assert parse_chains(chain[(hap, "to_ref")]) == flipped(parse_chains(chain[(hap, "from_ref")])), hap


def block_table(c):
    """a parsed chain -> [(t_start, q_start, size)] of its blocks"""
    out, t, q = [], c["t"][3], c["q"][3]
    for size, dt, dq in c["blocks"]:
        out.append((t, q, size))
        t += size + dt; q += size + dq
    out.append((t, q, c["last"]))
    return out


# ---- 1. the model itself ----
WORKED_REF = "ACGTACGTAC"
WORKED_EDITS = [(0, "D", "", 3), (1, "D", "", 3), (3, "I", "TT", 3), (4, "D", "", 3), (5, "D", "", 3), (7, "S", "A", 3), (9, "I", "G", 3)]
WORKED_FROM = b"chain 6 c 10 + 2 10 c 9 + 0 8 1\n2\t2\t2\n4\n\n"
WORKED_TO = b"chain 6 c 9 + 0 8 c 10 + 2 10 1\n2\t2\t2\n4\n\n"


def check_model():
    r0, blocks = chain_blocks(10, WORKED_EDITS, 0)
    assert (r0, blocks) == (2, [(2, 2, 2), (4, 0, 1)]) and len(H.apply_edits(WORKED_REF, WORKED_EDITS, 0)) == 9
    assert format_chain("c", 10, r0, blocks, "from_ref", 1) == WORKED_FROM and format_chain("c", 10, r0, blocks, "to_ref", 1) == WORKED_TO
    assert chain_blocks(4, [(q, "D", "", 1) for q in range(4)], 0) == (0, []) and chain_blocks(4, [(q, "D", "", 1) for q in range(4)], 1) == (0, [(4, 0, 0)])
    assert chain_blocks(5, [(1, "I", "A", 3), (2, "D", "", 3)], 0) == (0, [(2, 1, 1), (2, 0, 0)])      # an insertion directly followed by a deletion: one gap
    assert parse_chains(WORKED_FROM) == flipped(parse_chains(WORKED_TO))
    assert block_table(parse_chains(WORKED_FROM)[0]) == [(2, 0, 2), (6, 4, 4)]


def check_formatter(lib):
    """the exported formatter on the worked example, and what it refuses"""
    blocks = [(2, 2, 2), (4, 0, 1)]
    assert api.chain_format("c", 10, 2, blocks, "from_ref", 1, lib) == WORKED_FROM and api.chain_format("c", 10, 2, blocks, "to_ref", 1, lib) == WORKED_TO
    assert api.chain_format("c", 10, 2, blocks, api.CHAIN_FROM_REF, 7, lib) == WORKED_FROM.replace(b" 1\n", b" 7\n", 1)
    blk = (api.ChainBlock * 2)(*[api.ChainBlock(*b) for b in blocks])
    assert lib.dwgsim_hip_chain_format(b"c", 10, 2, blk, 2, 1, 1, None, 0) == len(WORKED_FROM)
    assert lib.dwgsim_hip_chain_format(b"c", 10, 2, blk, 0, 1, 1, None, 0) == -1      # DWGSIM_HIP_ERR_ARG: no block
    assert lib.dwgsim_hip_chain_format(b"c", 10, 2, blk, 2, 2, 1, None, 0) == -1      # no such direction
    assert lib.dwgsim_hip_chain_format(b"c", 11, 2, blk, 2, 1, 1, None, 0) == -1      # the blocks do not add up to l
    assert lib.dwgsim_hip_chain_format(None, 10, 2, blk, 2, 1, 1, None, 0) == -1


# ---- 2. unmutated contigs: one block each ----
def check_unmutated(lib):
    contigs = H.layout_contigs()
    want = expected(contigs)
    for d in DIRECTIONS:
        assert want[(0, d)] == b"".join(f"chain {len(a)} {n} {len(a)} + 0 {len(a)} {n} {len(a)} + 0 {len(a)} {k + 1}\n{len(a)}\n\n".encode() for k, (n, a) in enumerate(contigs))
    p = lambda: api.parse_flags("-z 3 -r 0 -M 2", lib)
    each = api.run_job(p(), contigs, lib=lib, group_bp=0, chain=True)
    one = api.run_job(p(), contigs, lib=lib, group_bp=1 << 30, chain=True)
    job = api.run_job_api(p(), contigs, devices=[0], gzip_on_gpu=False, group_bp=1 << 30, lib=lib, chain=True)
    assert each.chain == want and one.chain == want and job.chain == want
    assert [c["id"] for c in parse_chains(one.chain[(1, "to_ref")])] == list(range(1, 18))


# ---- 3. placed edits through a -m file ----
def placed_case_2():
    """Four contigs in one group.  As in hapfasta_common.placed_case the bases next to every edit are pinned so that the file-driven walk's left-justification
    moves nothing: a deletion run a .. b stays where the base in front of it differs from the run's last base (or the cell in front is mutated, or the run
    reaches the contig's end); an insertion behind cell p stays where the base of cell p - 1 differs from its last base (or cell p - 1 is mutated).  Every
    cell of a run and both its neighbours are pinned to letters, so that no N of synth() falls among them."""
    a, d, b, c = H.synth(61, 14000), H.synth(62, 300), H.synth(63, 13000), H.synth(64, 9000)
    pat = lambda q: "ACGT"[q & 3]

    def pin(arr, lo, hi, front=None):      # cells lo .. hi by pattern; the cell in front of lo differs from cell hi
        for q in range(max(lo - 1, 0), min(hi + 2, len(arr))):
            arr[q] = ord(pat(q))
        if lo > 0:
            arr[lo - 1] = ord(front or pat(hi + 1))

    dels = lambda lo, hi, mask=3: [(q, "D", "", mask) for q in range(lo, hi + 1)]
    edits = {"dA": [], "dD": [], "dB": [], "dC": []}
    pin(a, 0, 2); edits["dA"] += dels(0, 2)                              # a deletion run from cell 0
    pin(a, 15, 17); edits["dA"] += dels(15, 17, 1)                       # a deletion that starts at cell 15 (a thread's last cell), haplotype 1 only
    pin(a, 99, 103); a[99] = ord("A"); a[100] = ord("C"); a[103] = ord("T")
    edits["dA"] += [(100, "I", "TG", 3)] + dels(101, 103)                # an insertion directly followed by a deletion: both gap columns non-zero
    pin(a, 199, 203); edits["dA"] += dels(200, 202) + [(203, "I", "CA", 3)]      # an aligned INSERT cell directly behind a deletion
    pin(a, 4089, 4100); a[4089] = ord("G"); a[4094] = ord("T"); a[4095] = ord("A"); a[4099] = ord("C")
    edits["dA"] += dels(4090, 4094) + dels(4096, 4099)                   # one aligned cell, 4095, between two deletions
    pin(a, 13990, 13999); edits["dA"] += dels(13990, 13999)              # a deletion run to the contig's last cell
    edits["dD"] += dels(0, 299, 1)                                       # haplotype 1 of dD is deleted whole: no chain there, one block in haplotype 2
    for q in range(300):
        d[q] = ord(pat(q))
    pin(b, 16, 18); edits["dB"] += dels(16, 18)                          # a deletion that starts at cell 16 (a thread's first cell)
    pin(b, 4000, 12300); edits["dB"] += dels(4000, 12300)                # a homozygous deletion that covers two whole kernel blocks (4096 .. 12287)
    pin(c, 4089, 4101); c[4089] = ord("G"); c[4095] = ord("T"); c[4096] = ord("A"); c[4100] = ord("C")
    edits["dC"] += dels(4090, 4095) + dels(4097, 4100)                   # one aligned cell, 4096, between two deletions
    return [("dA", a), ("dD", d), ("dB", b), ("dC", c)], edits


def run_placed(lib, tmp_path, case, tag):
    contigs, edits = case
    path = os.path.join(str(tmp_path), tag + ".txt")
    with open(path, "w") as f:
        for name, arr in contigs:
            f.write(H.edits_to_txt(name, H.normalise(arr), edits[name]))
    res = api.run_job(api.parse_flags(f"-z 5 -M 2 -m {path}", lib), contigs, lib=lib, group_bp=1 << 30, chain=True, haplotypes=True, hap_width=0)
    for hap in (0, 1):      # the cells are the edits as written (nothing moved): the haplotype text is the model's
        assert res.haplotypes[hap] == H.expected(contigs, 0, edits, hap), (tag, hap)
    want = expected(contigs, edits)
    for key in KEYS:
        assert res.chain[key] == want[key], (tag, key)
    check_directions(res.chain)
    return res, want


def check_placed_edits(lib, tmp_path):
    res, _ = run_placed(lib, tmp_path, H.placed_case(), "placed")
    ca = parse_chains(res.chain[(0, "from_ref")])[0]
    assert (2091, 0, 3) in ca["blocks"] and (1, 0, 2) in ca["blocks"] and ca["q"][1] - ca["q"][4] == 3      # cells 2005 .. 4095 + GGT, cell 4096 + TA; TTC behind the last cell
    cb = parse_chains(res.chain[(1, "from_ref")])[1]
    assert (11, 0) in [(b[1], b[2]) for b in cb["blocks"]] and sum(b[2] for b in cb["blocks"]) == 6000


def check_placed_edits_2(lib, tmp_path):
    res, want = run_placed(lib, tmp_path, placed_case_2(), "placed2")
    h1, h2 = parse_chains(res.chain[(0, "from_ref")]), parse_chains(res.chain[(1, "from_ref")])
    assert [c["t"][0] for c in h1] == ["dA", "dB", "dC"] and [c["id"] for c in h1] == [1, 2, 3]      # dD has no chain in haplotype 1 ...
    assert [c["t"][0] for c in h2] == ["dA", "dD", "dB", "dC"] and [c["id"] for c in h2] == [1, 2, 3, 4] and h2[1]["blocks"] == [] and h2[1]["last"] == 300
    da, db, dc = h1
    assert da["t"][3] == 3 and da["t"][4] == 13990                       # the deletions at the contig's two ends are not part of the chain
    assert (3, 2) in [(b[1], b[2]) for b in da["blocks"]]                # the insertion directly followed by the deletion
    assert [b for b in db["blocks"] if b[1] == 8301] == [(4000 - 19, 8301, 0)]      # the kilobase deletion is one gap
    assert (1, 4, 0) in da["blocks"] and (1, 4, 0) in dc["blocks"]       # the single aligned cells
    assert len(da["blocks"]) + 1 == 7 and len(h2[0]["blocks"]) + 1 == 6 and len(db["blocks"]) + 1 == 3 and len(dc["blocks"]) + 1 == 3


# ---- 4. a random walk against the job's own mutations.txt ----
WALKS = H.RANDOM_WALKS + ("-z 13 -r 0.02 -R 0.5 -X 0.5 -N 200 -1 50 -2 50",)
WALK_IDS = ["substitutions", "indels", "mixed"]


def check_random_walk(lib, flags):
    contigs = [("walk", H.synth(21, 20000))]
    res = api.run_job(api.parse_flags(flags, lib), contigs, lib=lib, chain=True)
    edits = H.parse_mutations_txt(res.mutations_txt)
    assert len(edits["walk"]) > 200
    want = expected(contigs, edits)
    for key in KEYS:
        assert res.chain[key] == want[key], key
    n = len(parse_chains(res.chain[(0, "from_ref")])[0]["blocks"])
    assert n == 0 if " -R 0 " in flags else n > 50


# ---- 5. without the model: the chain against the haplotype FASTA ----
def check_against_fasta(lib, flags):
    """Over every block the haplotype text equals the reference but at the substitutions mutations.txt lists.  (The flag sets are RANDOM_WALKS': with mixed
    edits the reference's left-shift of a homozygous deletion can pass over a substituted cell, whose base then stays in the haplotype and leaves
    mutations.txt -- SURVEY "Hom-deletion left-shift"; mixed edits are compared without any list in check_against_truth_sam.)"""
    contigs = [("walk", H.synth(21, 20000)), ("walk2", H.synth(22, 9000))]
    res = api.run_job(api.parse_flags(flags, lib), contigs, lib=lib, group_bp=1 << 30, chain=True, haplotypes=True, hap_width=0)
    edits = H.parse_mutations_txt(res.mutations_txt)
    for hap in (0, 1):
        text = H.records(res.haplotypes[hap])
        chains = parse_chains(res.chain[(hap, "from_ref")])
        assert [c["t"][0] for c in chains] == [n for n, _ in contigs]
        for c, (name, arr) in zip(chains, contigs):
            ref, hp, l = H.normalise(arr), text[name], len(arr)
            subs = {pos for pos, kind, _, mask in edits.get(name, []) if kind == "S" and mask & (1 << hap)}
            assert c["t"][0] == c["q"][0] == name and c["t"][1] == l and c["q"][1] == len(hp) and c["q"][3] == 0
            for t0, q0, size in block_table(c):
                a, b = np.frombuffer(ref[t0:t0 + size].encode(), dtype=np.uint8), np.frombuffer(hp[q0:q0 + size].encode(), dtype=np.uint8)
                assert len(a) == len(b) == size
                assert {t0 + int(k) for k in np.nonzero(a != b)[0]} <= subs, (name, hap, t0)
            sizes = sum(b[0] for b in c["blocks"]) + c["last"]
            assert sizes + sum(b[2] for b in c["blocks"]) + (c["q"][1] - c["q"][4]) == len(hp)                 # ... + the inserted bases behind the last block
            assert sizes + sum(b[1] for b in c["blocks"]) + c["t"][3] + (l - c["t"][4]) == l                   # ... + the deleted cells at the two ends
    check_directions(res.chain)


# ---- 6. without the model: the chain against the truth SAM ----
def check_against_truth_sam(lib, haploid: bool):
    contigs = [("chrA", H.synth(31, 10000)), ("chrB", H.synth(32, 9500))]
    flags = "-e 0 -E 0 -y 0 -r 0.02 -R 0.3 -X 0.5 -N 2000 -1 70 -2 70 -z 17" + (" -H" if haploid else "")
    res = api.run_job(api.parse_flags(flags, lib), contigs, lib=lib, group_bp=1 << 30, truth_sam=True, haplotypes=True, hap_width=0, chain=True)
    if haploid:
        assert res.chain[(0, "from_ref")] == res.chain[(1, "from_ref")] and res.chain[(0, "to_ref")] == res.chain[(1, "to_ref")]
    else:
        assert res.chain[(0, "from_ref")] != res.chain[(1, "from_ref")]
    text = [H.records(res.haplotypes[q]) for q in (0, 1)]
    tables = [{c["t"][0]: block_table(c) for c in parse_chains(res.chain[(q, "from_ref")])} for q in (0, 1)]
    n = 0
    for line in res.truth_sam.decode().splitlines():
        f = line.split("\t")
        if int(f[1]) & 4:
            continue
        hap = int([t for t in f[11:] if t.startswith("HP:i:")][0][5:]) - 1
        pos, cigar, seq = int(f[3]) - 1, f[5], f[9]
        hit = [(t0, q0) for t0, q0, size in tables[hap][f[2]] if t0 <= pos < t0 + size]
        assert len(hit) == 1, line      # POS lies inside a block
        at = hit[0][1] + pos - hit[0][0]
        k = 0
        while cigar[k].isdigit():
            k += 1
        if cigar[k] == "I":             # the read begins inside the bases inserted in front of POS
            at -= int(cigar[:k])
        assert text[hap][f[2]][at:at + len(seq)] == seq, line
        n += 1
    assert n == 4000


# ---- 8. the job level against the context level ----
def check_levels(lib, tmp_path):
    contigs, flags = H.levels_case(tmp_path)
    ctx_level = api.run_job(api.parse_flags(flags, lib), contigs, lib=lib, group_bp=0, chain=True)
    job_level = api.run_job_api(api.parse_flags(flags, lib), contigs, devices=[0], gzip_on_gpu=False, batch_pairs=150, group_bp=8000, lib=lib, chain=True)
    assert set(job_level.chain) == set(KEYS) and job_level.chain == ctx_level.chain and job_level.chain_threads == 1
    for key in KEYS:
        chains = parse_chains(job_level.chain[key])
        side = "t" if key[1] == "from_ref" else "q"
        assert [c[side][0] for c in chains] == ["g1", "g2", "g3"] and [c["id"] for c in chains] == [1, 2, 3], key      # allN and tiny are passed over; the ids run across the groups
    assert job_level.mutations_txt == ctx_level.mutations_txt and job_level.streams == ctx_level.streams
    both = api.run_job_api(api.parse_flags(flags, lib), contigs, devices=[0], gzip_on_gpu=False, batch_pairs=150, group_bp=8000, lib=lib, chain=True, haplotypes=True)
    assert both.chain == job_level.chain and both.streams == job_level.streams      # with the haplotype sink as without it
    plain = api.run_job_api(api.parse_flags(flags, lib), contigs, devices=[0], gzip_on_gpu=False, batch_pairs=150, group_bp=8000, lib=lib)
    assert plain.chain == {} and plain.streams == job_level.streams and plain.mutations_txt == job_level.mutations_txt and plain.mutations_vcf == job_level.mutations_vcf
    plain_ctx = api.run_job(api.parse_flags(flags, lib), contigs, lib=lib, group_bp=0)
    assert plain_ctx.chain == {} and plain_ctx.streams == ctx_level.streams and plain_ctx.mutations_txt == ctx_level.mutations_txt


# ---- 9. the command line ----
def check_cli(lib, cli, tmp_path, gzip_mode):
    contigs, flags = H.levels_case(tmp_path)
    fa = os.path.join(str(tmp_path), "in.fa")
    with open(fa, "w") as f:
        for name, arr in contigs:
            s = bytes(bytearray(arr)).decode()
            f.write(f">{name}\n" + "".join(s[i:i + 70] + "\n" for i in range(0, len(s), 70)))
    base = {k: v for k, v in os.environ.items() if not k.startswith("DWGSIM_HIP_HAPLOTYPES") and k != "DWGSIM_HIP_CHAIN"}
    base.update(DWGSIM_HIP_GZIP=gzip_mode, DWGSIM_HIP_GROUP_BP="8000", DWGSIM_HIP_BATCH="150")
    outs = {}
    for tag, extra in (("on", {"DWGSIM_HIP_CHAIN": "1"}), ("both", {"DWGSIM_HIP_CHAIN": "yes", "DWGSIM_HIP_HAPLOTYPES": "1"}), ("off", {}), ("zero", {"DWGSIM_HIP_CHAIN": "0"}),
                       ("pre", {"DWGSIM_HIP_CHAIN": "1"})):
        prefix = os.path.join(str(tmp_path), tag)
        subprocess.run([cli] + flags.split() + (["-P", "px"] if tag == "pre" else []) + [fa, prefix], check=True, stderr=subprocess.DEVNULL, env=dict(base, **extra), timeout=600)
        outs[tag] = {}
        for name in sorted(os.listdir(str(tmp_path))):
            if name.startswith(tag + "."):
                data = open(os.path.join(str(tmp_path), name), "rb").read()
                outs[tag][name[len(tag):]] = gzip.decompress(data) if name.endswith(".gz") else data
    want = api.run_job(api.parse_flags(flags, lib), contigs, lib=lib, group_bp=0, fetch=False, chain=True).chain
    for tag in ("on", "both", "pre"):      # (a -P prefix stands in the read names alone)
        assert {k: outs[tag][FILES[k]] for k in KEYS} == want, tag
    others = outs["off"]
    assert len(others) == 5 and not any(k.endswith(".chain") for k in others) and outs["zero"] == others
    assert {k: v for k, v in outs["on"].items() if not k.endswith(".chain")} == others and len(outs["on"]) == 9
    assert {k: v for k, v in outs["both"].items() if not k.endswith(".chain") and not k.startswith(".hap")} == others and len(outs["both"]) == 11


# ---- 10. argument and state errors ----
def check_errors(lib):
    import ctypes as C
    p = api.parse_flags("-z 3 -r 0.01 -R 0.5 -M 2", lib)
    with api.Context(p, 0, lib) as ctx:
        h = ctx.add_contigs([("e", H.synth(51, 5000))])
        n, r0 = C.c_uint64(0), C.c_int64(0)
        assert lib.dwgsim_hip_haplotype_chain(ctx.h, h, 0, C.byref(n)) == -6      # DWGSIM_HIP_ERR_STATE: before the walk
        assert lib.dwgsim_hip_chain_blocks(ctx.h, h, 0, C.byref(n), C.byref(r0), None, 0) == -6
        ctx.mutate(h)
        assert lib.dwgsim_hip_chain_blocks(ctx.h, h, 0, C.byref(n), C.byref(r0), None, 0) == -6      # walked, not built
        assert lib.dwgsim_hip_haplotype_chain(ctx.h, h, 2, C.byref(n)) == -1       # DWGSIM_HIP_ERR_ARG
        assert lib.dwgsim_hip_haplotype_chain(ctx.h, h, -1, C.byref(n)) == -1
        assert lib.dwgsim_hip_haplotype_chain(ctx.h, h + 1, 0, C.byref(n)) == -1   # no such contig
        assert lib.dwgsim_hip_haplotype_chain(ctx.h, h, 0, C.byref(n)) == 0 and n.value > 1
        total = n.value
        assert lib.dwgsim_hip_chain_blocks(ctx.h, h, 0, C.byref(n), C.byref(r0), None, 0) == 0 and n.value == total
        assert lib.dwgsim_hip_chain_blocks(ctx.h, h, 2, C.byref(n), None, None, 0) == -1 and lib.dwgsim_hip_chain_blocks(ctx.h, h + 1, 0, C.byref(n), None, None, 0) == -1
        assert lib.dwgsim_hip_chain_blocks(ctx.h, h, 0, None, None, None, 1) == -1  # a capacity without an array
        assert lib.dwgsim_hip_chain_blocks(ctx.h, h, 1, C.byref(n), None, None, 0) == -6      # haplotype 2 has not been built
        first = ctx.haplotype_chain(h, 0)
        assert len(first[1]) == total and ctx.haplotype_chain(h, 0) == first, "the same call twice"
        ctx.mutate(h)                                                               # walked again: the blocks are gone
        assert lib.dwgsim_hip_chain_blocks(ctx.h, h, 0, C.byref(n), None, None, 0) == -6
        assert ctx.haplotype_chain(h, 0) == first                                   # (the same seed: the same walk)
    # the job's sink: after prepare it is refused
    cb = api.CHAIN_CB(lambda user, hap, direction, data, size: 0)
    sink = api.JobSink(None, api.MUT_CB(lambda *a: 0), api.READS_CB(lambda *a: 0), api.MSG_CB(lambda u, m: None), api.READS_AT_CB())
    opt = api.JobOptions(0, 1, 0, 0, 0)
    err = C.c_int(0)
    devs = (C.c_int * 1)(0)
    job = lib.dwgsim_hip_job_create(C.byref(p), devs, 1, C.byref(sink), C.byref(opt), C.byref(err))
    assert job
    try:
        names, lens = (C.c_char_p * 1)(b"e"), (C.c_int64 * 1)(5000)
        assert lib.dwgsim_hip_job_set_contig_table(job, names, lens, 1) == 0
        assert lib.dwgsim_hip_job_set_chain_sink(job, cb, None) == 0
        assert lib.dwgsim_hip_job_prepare(job, None) == 0
        assert lib.dwgsim_hip_job_set_chain_sink(job, cb, None) == -6
        assert lib.dwgsim_hip_job_finish(job) == 0
    finally:
        lib.dwgsim_hip_job_destroy(job)
