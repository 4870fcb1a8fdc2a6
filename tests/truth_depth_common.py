"""The truth VCF and the counters behind it (include/dwgsim_hip.h dwgsim_hip_set_truth_depth; DESIGN.md "6f"; the rule: the head comment of k_truth_depth in
dwgsim_amd/csrc/dw_truth.hpp): a plain-Python model and the cases tests/test_emu_truth_depth.py (CPU emulation) and tests/test_gpu_truth_depth.py (device) both
run.  Every check_* function takes the loaded library.

The model replays no random numbers and shares no code with the product.  It takes the truth SAM of the same run -- which truth_sam_common.check_sam holds to the
FASTQ text and to mutations.txt in the same test -- and mutations.txt (hapfasta_common.parse_mutations_txt).  Every mapped record's CIGAR is walked from POS on
haplotype HP: an M cell counts, unless that haplotype inserts there and the I run behind it is missing or shorter than the insertion; every D cell counts; I
runs count nowhere (a leading I belongs to a cell left of POS whose own base the read does not hold).  The counters are compared with the fetched ones cell by
cell, then GT:AD:DP of every line of the truth VCF with what the rule gives."""
import os
import subprocess

import numpy as np

import truth_sam_common as T
from dwgsim_amd import api
from hapfasta_common import edits_to_txt, normalise, parse_mutations_txt, synth

ERR_ARG, ERR_UNSUP, ERR_STATE = -1, -4, -6


# ---- the model ----
def model_add(counts: dict, cells, rec):
    """one mapped record (pos 1-based, cigar, hap 0 / 1) into counts = {listed cell: [n1, n2]}; cells = ({cell: (kind, bases)} of haplotype 1, of haplotype 2)"""
    h, c, ops = rec["hap"], rec["pos"] - 1, T.parse_cigar(rec["cigar"])
    for k, (n, o) in enumerate(ops):
        if o == "I":
            continue
        for q in range(c, c + n):
            if q not in counts:
                assert o == "M", "a deleted cell is a listed cell"
                continue
            if o == "M":
                kind, ins = cells[h].get(q, ("", ""))
                if kind == "I" and not (q == c + n - 1 and k + 1 < len(ops) and ops[k + 1] == (len(ins), "I")):
                    continue      # the insertion is not in the read, or not all of it
            counts[q][h] += 1
        c += n


def sam_records(sam: bytes):
    """the mapped records of a truth SAM: rname, pos, cigar, hap, and the span lo .. hi the CIGAR covers on the reference (0-based)"""
    out = []
    for line in sam.decode().splitlines():
        f = line.split("\t")
        if int(f[1]) & 4:
            continue
        assert f[11] in ("HP:i:1", "HP:i:2")
        r = dict(rname=f[2], pos=int(f[3]), cigar=f[5], hap=int(f[11][-1]) - 1)
        r["lo"] = r["pos"] - 1
        r["hi"] = r["lo"] + sum(n for n, o in T.parse_cigar(r["cigar"]) if o in "MD") - 1
        r["ops"] = T.parse_cigar(r["cigar"])
        out.append(r)
    return out


def model_counts(sam: bytes, edits: dict, extra=None):
    """{contig: (listed cells ascending, uint64 [cells, 2])}: edits = {contig: [(pos, kind, bases, mask)]}; extra = {contig: cells that are listed but print no
    line in mutations.txt (a reference code outside ACGT)}"""
    counts, cells = {}, {}
    for name in set(edits) | set(extra or {}):
        counts[name] = {pos: [0, 0] for pos, _, _, _ in edits.get(name, [])}
        counts[name].update({pos: [0, 0] for pos in (extra or {}).get(name, [])})
        cells[name] = (T.hap_cells(edits.get(name, []), 0), T.hap_cells(edits.get(name, []), 1))
    for r in sam_records(sam):
        if r["rname"] in counts:
            model_add(counts[r["rname"]], cells[r["rname"]], r)
    return {name: (sorted(c), np.array([c[q] for q in sorted(c)], dtype=np.uint64).reshape(len(c), 2)) for name, c in counts.items()}


def sample_column(pl: int, n, other_mutated: bool) -> str:
    """GT:AD:DP of a record of phase pl from the counters n = (n1, n2) of its cell"""
    n1, n2 = int(n[0]), int(n[1])
    if pl == 3:
        return f"1|1:0,{n1 + n2}:{n1 + n2}"
    alt, ref = (n1, n2) if pl == 1 else (n2, n1)
    return f"{'1|0' if pl == 1 else '0|1'}:{0 if other_mutated else ref},{alt}:{n1 + n2}"


def check_model():
    """the model on cases small enough to write out: cell 5 of haplotype 1 carries the insertion TT, cells 2 and 3 are deleted on both, cell 7 is a SNP of haplotype 2"""
    edits = [(2, "D", "", 3), (3, "D", "", 3), (5, "I", "TT", 1), (7, "S", "A", 2)]
    cells = (T.hap_cells(edits, 0), T.hap_cells(edits, 1))

    def run(recs):
        counts = {2: [0, 0], 3: [0, 0], 5: [0, 0], 7: [0, 0]}
        for pos, cigar, hap in recs:
            model_add(counts, cells, dict(pos=pos, cigar=cigar, hap=hap))
        return [counts[q] for q in (2, 3, 5, 7)]
    assert run([(1, "2M2D2M2I2M", 0)]) == [[1, 0], [1, 0], [1, 0], [1, 0]]      # spans the deletion run and the whole insertion
    assert run([(1, "2M2D4M", 1)]) == [[0, 1], [0, 1], [0, 1], [0, 1]]          # haplotype 2 has no insertion at cell 5: the cell counts as it is
    assert run([(5, "2M1I", 0)]) == [[0, 0], [0, 0], [0, 0], [0, 0]]            # ends inside the insertion (one base of two): cell 5 is left out
    assert run([(5, "2M", 0)]) == [[0, 0], [0, 0], [0, 0], [0, 0]]              # ends on the cell's own base: none of the insertion
    assert run([(5, "2M2I", 0)]) == [[0, 0], [0, 0], [1, 0], [0, 0]]            # ends behind the last inserted base: all of it
    assert run([(7, "1I2M", 0)]) == [[0, 0], [0, 0], [0, 0], [1, 0]]            # starts with I (cells 6 and 7 behind it): cell 5, which carries the insertion, lies left of POS and is left out
    assert run([(5, "1M", 1), (1, "2M", 0)]) == [[0, 0], [0, 0], [0, 0], [0, 0]]          # reads on unlisted cells only
    assert run([(2, "1M2D1M", 0), (2, "1M2D1M", 0), (2, "1M2D1M", 1)]) == [[2, 1], [2, 1], [0, 0], [0, 0]]      # the deletion run: every D cell, per haplotype
    assert sample_column(3, (4, 5), False) == "1|1:0,9:9" and sample_column(1, (4, 5), False) == "1|0:5,4:9"
    assert sample_column(2, (4, 5), False) == "0|1:4,5:9" and sample_column(2, (4, 5), True) == "0|1:0,5:9"


# ---- a run and its check ----
def run_ctx(lib, flags: str, contigs, truth_sam: bool = True, **kw):
    return api.run_job(api.parse_flags(flags, lib), contigs, lib=lib, truth_sam=truth_sam, truth_vcf=True, **kw)


def strip_truth_vcf(text: bytes) -> bytes:
    """a truth VCF without what it adds: the three ##FORMAT lines and the last two columns of every other line that has them"""
    out = []
    for line in text.decode().split("\n")[:-1]:
        if line.startswith("##FORMAT="):
            continue
        if not line.startswith("##"):
            f = line.split("\t")
            assert len(f) == 10 and (f[8:] == ["FORMAT", "dwgsim"] if line.startswith("#") else f[8] == "GT:AD:DP"), line
            line = "\t".join(f[:8])
        out.append(line + "\n")
    return "".join(out).encode()


def check_vcf(tvcf: bytes, model: dict, edits: dict):
    """GT:AD:DP of every record against the model's counters at the record's cell; returns the records as (contig, cell, pl, mt, sample)"""
    recs = []
    at = {name: {q: k for k, q in enumerate(pos)} for name, (pos, _) in model.items()}
    for line in tvcf.decode().splitlines():
        f = line.split("\t")
        assert len(f) == 10 and f[8] == "GT:AD:DP", line
        info = dict(kv.split("=") for kv in f[7].split(";"))
        pl, mt = int(info["pl"]), info["mt"]
        cell = int(f[1]) if mt == "DELETE" else int(f[1]) - 1      # a deletion is anchored at the base in front of its first deleted cell
        n = model[f[0]][1][at[f[0]][cell]]
        other = [e for e in edits.get(f[0], []) if e[0] == cell and pl != 3 and e[3] & (2 if pl == 1 else 1)]
        assert f[9] == sample_column(pl, n, bool(other)), (line, n)
        recs.append((f[0], cell, pl, mt, f[9]))
    return recs


def check_result(lib, res, contigs, paired: bool, exact: bool, edits=None, extra=None, prefix: str = ""):
    """a run with the truth SAM and the truth VCF: the SAM against FASTQ and mutations.txt, the counters against the model, the VCF against the counters.
    edits: what a -m file placed, where mutations.txt cannot say it (one line per cell, two edits at one): the SAM and the model are then held to these"""
    txt = res.mutations_txt if edits is None else "".join(edits_to_txt(n, normalise(a), [e]) for n, a in contigs for e in sorted(edits.get(n, []))).encode()
    st = T.check_sam(res.truth_sam, res.streams, contigs, txt, paired, exact, prefix)
    edits = edits if edits is not None else parse_mutations_txt(res.mutations_txt)
    model = model_counts(res.truth_sam, edits, extra)
    for name, got in res.truth_depth.items():
        want = model.get(name, ([], np.zeros((0, 2), dtype=np.uint64)))[1]
        assert got.shape == want.shape and (got == want).all(), (name, np.argwhere(got != want)[:5] if got.shape == want.shape else (got.shape, want.shape))
    assert set(model) <= set(res.truth_depth)
    recs = check_vcf(res.truth_vcf, model, edits)
    assert strip_truth_vcf(api.truth_vcf_header(contigs, lib) + res.truth_vcf) == res.mutations_vcf
    return st, model, recs


def same_counts(a, b):
    assert set(a.truth_depth) == set(b.truth_depth)
    for name in a.truth_depth:
        assert (a.truth_depth[name] == b.truth_depth[name]).all(), name
    assert a.truth_vcf == b.truth_vcf


# ---- 1. random walks (and 10: the coverage invariant) ----
WALK = "-z 17 -r 0.02 -R 0.5 -X 0.5 -N 2000"
WALK_KINDS = {"paired": " -1 100 -2 100 -e 0 -E 0", "paired50": " -1 50 -2 50 -e 0 -E 0", "single": " -1 50 -2 0 -e 0 -E 0", "haploid": " -1 100 -2 100 -e 0 -E 0 -H",
              "errors": " -1 100 -2 100"}


def check_random_walk(lib, kind: str):
    contigs = [("walk", synth(31, 5000))]
    flags = WALK + WALK_KINDS[kind]
    res = run_ctx(lib, flags, contigs)
    st, model, recs = check_result(lib, res, contigs, kind != "single", kind != "errors")
    pos, n = model["walk"]
    assert len(pos) > 100 and n.sum() > 10 * len(pos) and st.with_indel > 0
    kinds = {(mt, pl) for _, _, pl, mt, _ in recs}
    if kind == "haploid":
        assert {pl for _, pl in kinds} == {3}
    else:
        assert kinds >= {(mt, pl) for mt in ("SUBSTITUTE", "INSERT", "DELETE") for pl in (1, 2, 3)}, kinds
    # the coverage invariant: a homozygous SNP is in every read whose span covers its cell
    sam = sam_records(res.truth_sam)
    lo, hi = np.array([r["lo"] for r in sam]), np.array([r["hi"] for r in sam])
    hom = [(cell, s) for _, cell, pl, mt, s in recs if pl == 3 and mt == "SUBSTITUTE"]
    assert len(hom) >= 5
    for cell, s in hom:
        assert int(s.split(":")[2]) == int(((lo <= cell) & (cell <= hi)).sum()), cell
    if kind == "errors":      # the errors move no read: the counters are those of the error-free run
        same_counts(res, run_ctx(lib, WALK + WALK_KINDS["paired"], contigs))


# ---- 2. placed edits through -m ----
def placed_case():
    """One contig.  A 40-base insertion and a 300-base deletion on haplotype 1, a homozygous insertion, a SNP on each haplotype, a substitution on haplotype 1 and a
    deletion on haplotype 2 at one cell, an edit at cell 0 and one at the last cell.  The neighbours of every indel are pinned so that left-justification moves
    nothing (the test asserts that the run's mutations.txt gives the edits back)."""
    a = synth(7, 6000)
    pins = {0: "A", 5999: "G", 5998: "A", 999: "A", 1000: "C", 1001: "G", 1999: "A", 2299: "C", 2300: "G", 2999: "A", 3000: "T", 3001: "A", 3500: "A", 3600: "C", 3999: "A", 4000: "G", 4001: "T"}
    pins.update({q: "ACGT"[q & 3] for q in range(2000, 2299)})
    for q, ch in pins.items():
        a[q] = ord(ch)
    big = "".join("ACGT"[(7 * q + q // 5) & 3] for q in range(39)) + "G"
    edits = {"cA": [(0, "S", "T", 3), (5999, "S", "C", 1), (1000, "I", big, 1), (3000, "I", "CCG", 3), (3500, "S", "G", 1), (3600, "S", "T", 2),
                    (4000, "S", "A", 1), (4000, "D", "", 2)] + [(q, "D", "", 1) for q in range(2000, 2300)]}
    return [("cA", a)], edits


def check_placed(lib, tmp_path):
    contigs, edits = placed_case()
    path = os.path.join(str(tmp_path), "placed.txt")
    ref = normalise(contigs[0][1])
    with open(path, "w") as f:      # (the two edits of cell 4000 as two lines, one per haplotype)
        f.write(edits_to_txt("cA", ref, [e for e in edits["cA"] if e != (4000, "D", "", 2)]))
        f.write(edits_to_txt("cA", ref, [(4000, "D", "", 2)]))
    res = run_ctx(lib, f"-z 5 -e 0 -E 0 -y 0 -N 3000 -1 50 -2 50 -m {path}", contigs)
    got = parse_mutations_txt(res.mutations_txt)["cA"]
    assert sorted(e for e in got if e[0] != 4000) == sorted(e for e in edits["cA"] if e[0] != 4000), "the walk moved a placed edit"
    assert [e[0] for e in got].count(4000) == 1      # one line for the cell that carries two edits: the model takes the edits as they were placed
    st, model, recs = check_result(lib, res, contigs, True, True, edits=edits)
    sam = [r for r in sam_records(res.truth_sam) if r["hap"] == 0]
    short_tail = [r for r in sam if r["hi"] == 1000 and (r["ops"][-1][1] == "M" or (r["ops"][-1][1] == "I" and r["ops"][-1][0] < 40))]
    lead = [r for r in sam if r["ops"][0][1] == "I" and r["lo"] == 1001]
    covering = [r for r in sam if r["lo"] <= 1000 <= r["hi"]]      # (a lead's span starts behind cell 1000: none of them is here)
    assert len(short_tail) >= 1 and any(r["ops"][-1][1] == "I" for r in short_tail) and len(lead) >= 1 and len(covering) > len(short_tail), (len(short_tail), len(lead), len(covering))
    pos, n = model["cA"]
    k = pos.index(1000)
    assert int(res.truth_depth["cA"][k][0]) == int(n[k][0]) == len(covering) - len(short_tail)      # both kinds are left out
    by_cell = {cell: s for _, cell, _, _, s in recs}
    assert by_cell[4000].startswith("1|0:0,")      # haplotype 2 carries another edit there: no reference allele
    d = [k for k, q in enumerate(pos) if 2000 <= q < 2300]
    assert len({int(n[k][0]) for k in d}) == 1 and int(n[d[0]][0]) >= 1      # a deletion is spanned whole: every cell of the run has the same count
    assert by_cell[2000].split(":")[1].split(",")[1] == str(int(n[d[0]][0])) and sum(1 for _, _, _, mt, _ in recs if mt == "DELETE") == 1      # (the deletion of cell 4000 stands behind the substitution there and has no record)
    assert 0 in by_cell and 5999 in by_cell


# ---- 3. random reads, regions, listed cells without a record ----
def check_random_reads(lib):
    contigs = [("rr", synth(33, 4000))]
    res = run_ctx(lib, "-z 9 -r 0.02 -R 0.3 -N 1500 -1 50 -2 50 -e 0 -E 0 -y 0.2", contigs)
    st, model, _ = check_result(lib, res, contigs, True, True)
    assert 0 < st.mapped < st.records


def check_regions(lib, tmp_path):
    contigs = [("surf", synth(41, 6000))]
    bed = os.path.join(str(tmp_path), "two.bed")
    with open(bed, "w") as f:
        f.write("surf\t500\t2000\nsurf\t3000\t5000\n")
    res = run_ctx(lib, f"-z 29 -r 0.02 -R 0.3 -X 0.4 -N 1500 -1 50 -2 50 -e 0 -E 0 -x {bed}", contigs)
    _, model, _ = check_result(lib, res, contigs, True, True)
    pos, n = model["surf"]
    outside = [k for k, q in enumerate(pos) if 2200 <= q < 2800]
    assert outside and all(int(n[k].sum()) == 0 for k in outside) and n.sum() > 0      # no read lies between the regions


def check_non_acgt(lib, tmp_path):
    """a substitution placed on a cell of an N run: the cell is listed and counted, and prints no record"""
    a = synth(51, 4000)
    ref = normalise(a)
    n_cell = next(q for q in range(100, 3900) if ref[q - 1:q + 2] == "NNN")
    path = os.path.join(str(tmp_path), "n.txt")
    edits = {"nn": [(50, "S", "ACGT"[("ACGT".index(ref[50]) + 1) & 3] if ref[50] != "N" else "A", 3), (3950, "D", "", 1)]}
    a[50] = ord("A") if ref[50] == "N" else a[50]
    a[3949], a[3950], a[3951] = ord("A"), ord("C"), ord("G")
    ref = normalise(a)
    edits = {"nn": [(50, "S", "ACGT"[("ACGT".index(ref[50]) + 1) & 3], 3), (3950, "D", "", 1)]}
    with open(path, "w") as f:
        f.write(edits_to_txt("nn", ref, edits["nn"]))
        f.write(f"nn\t{n_cell + 1}\tN\tA\t3\n")
    contigs = [("nn", a)]
    res = run_ctx(lib, f"-z 3 -e 0 -E 0 -N 1500 -1 50 -2 50 -n 50 -m {path}", contigs)
    assert sorted(parse_mutations_txt(res.mutations_txt)["nn"]) == sorted(edits["nn"])      # no line for the N cell
    _, model, recs = check_result(lib, res, contigs, True, False, extra={"nn": [n_cell]})
    pos, n = model["nn"]
    assert len(res.truth_depth["nn"]) == 3 and int(n[pos.index(n_cell)].sum()) > 0 and len(recs) == 2


# ---- 4. several contigs resident together ----
def group_case():
    return [("g1", synth(61, 3000)), ("tiny", synth(63, 100)), ("g2", synth(62, 5000)), ("g3", synth(64, 2500))], "-z 23 -r 0.02 -R 0.3 -N 1800 -1 50 -2 50 -e 0 -E 0"


def check_group(lib):
    contigs, flags = group_case()
    together = run_ctx(lib, flags, contigs, group_bp=1 << 30)
    st, model, _ = check_result(lib, together, contigs, True, True)
    assert set(together.truth_depth) == {"g1", "g2", "g3"} and all(model[n][1].sum() > 0 for n in model)      # `tiny` is passed over: no counters, no records
    same_counts(together, run_ctx(lib, flags, contigs, group_bp=0))
    return together


# ---- 5. one contig in several batches, and on two contexts ----
def check_batches(lib):
    contigs, flags = group_case()
    whole = run_ctx(lib, flags, contigs, group_bp=1 << 30)
    for bp in (129, 257, 700):
        same_counts(whole, run_ctx(lib, flags, contigs, group_bp=1 << 30, batch_pairs=bp))
    # the same contig as two read-index halves on two contexts, summed on the host
    contigs, flags = [("half", synth(65, 4000))], "-z 23 -r 0.02 -R 0.3 -N 1500 -1 50 -2 50 -e 0 -E 0 -y 0"
    p = api.parse_flags(flags, lib)
    one = run_ctx(lib, flags, contigs)
    parts = []
    for first, n in ((0, 700), (700, 800)):
        with api.Context(p, 0, lib) as ctx:
            ctx.set_truth_depth(True)
            h = ctx.add_contigs(contigs)
            ctx.mutate(h)
            ctx.simulate(h, first, n, 0, 0)
            parts.append(ctx.truth_depth(h))
            if first:
                text = ctx.truth_vcf_via_list(h, [parts[0] + parts[1]])
    assert ((parts[0] + parts[1]) == one.truth_depth["half"]).all() and parts[0].sum() > 0 and parts[1].sum() > 0
    assert b"".join(text) == one.truth_vcf


# ---- 6. the forced second run ----
def check_rerun(lib):
    contigs = [("re", synth(66, 4000))]
    flags = "-z 41 -r 0.02 -R 0.5 -X 0.5 -N 1200 -1 50 -2 50"
    capped = run_ctx(lib, flags, contigs, truth_md=True, debug_options={"truth_cap": 64})
    free = run_ctx(lib, flags, contigs, truth_md=True)
    assert capped.truth_reruns >= 1 and free.truth_reruns == 0 and capped.truth_sam == free.truth_sam
    same_counts(capped, free)
    assert capped.truth_depth["re"].sum() > 0


# ---- 7. the feature without the truth SAM ----
def check_alone(lib):
    contigs, flags = group_case()
    both = run_ctx(lib, flags, contigs, group_bp=1 << 30)
    alone = run_ctx(lib, flags, contigs, truth_sam=False, group_bp=1 << 30)
    assert alone.truth_sam == b"" and alone.streams == both.streams
    same_counts(both, alone)
    p = api.parse_flags(flags, lib)
    with api.Context(p, 0, lib) as ctx:
        ctx.set_truth_depth(True)
        h = ctx.add_contigs([contigs[0]])
        ctx.mutate(h)
        assert ctx.truth_depth(h).sum() == 0      # before any batch: the cells, all zero
        b = ctx.simulate(h, 0, 300, 0, 0)
        assert b.sam_bytes == 0 and b.sam_gz_bytes == 0 and not b.sam_dev_ptr and ctx.truth_depth(h).sum() > 0
        first = ctx.truth_depth(h)
        ctx.simulate(h, 0, 300, 0, 1)      # the same reads once more: the counters run on
        assert (ctx.truth_depth(h) == 2 * first).all()
        ctx.mutate(h)                      # a new walk: they start again
        assert ctx.truth_depth(h).sum() == 0


# ---- 8. the feature off ----
def check_off(lib):
    import ctypes as C
    contigs, flags = group_case()
    p = api.parse_flags(flags, lib)
    with api.Context(p, 0, lib) as ctx:
        h = ctx.add_contigs([contigs[0]])
        ctx.mutate(h)
        ctx.simulate(h, 0, 100, 0, 0)
        buf = (C.c_uint64 * 16)()
        assert lib.dwgsim_hip_truth_depth_fetch(ctx.h, h, buf, 8) == ERR_ARG and lib.dwgsim_hip_truth_depth_fetch(ctx.h, h, None, 0) == ERR_ARG
        ctx.simulate_async(h, 0, 100, 0, 1)
        assert lib.dwgsim_hip_set_truth_depth(ctx.h, 1) == ERR_STATE      # a slot is pending
        ctx.wait(1)
        ctx.set_truth_depth(True)
        assert lib.dwgsim_hip_truth_depth_fetch(ctx.h, h, None, 0) > 0 and lib.dwgsim_hip_truth_depth_fetch(ctx.h, h + 7, None, 0) == ERR_ARG
    on = run_ctx(lib, flags, contigs, group_bp=1 << 30)
    off = api.run_job(api.parse_flags(flags, lib), contigs, lib=lib, truth_sam=True, group_bp=1 << 30)
    assert off.truth_vcf == b"" and off.truth_depth == {}
    assert off.streams == on.streams and off.mutations_txt == on.mutations_txt and off.mutations_vcf == on.mutations_vcf and off.truth_sam == on.truth_sam
    for f in ("-z 3 -N 10 -c 1", "-z 3 -N 10 -c 2 -f TACG -2 0"):
        with api.Context(api.parse_flags(f, lib), 0, lib) as ctx:
            assert lib.dwgsim_hip_set_truth_depth(ctx.h, 1) == ERR_UNSUP and b"true read depth" in lib.dwgsim_hip_last_error(ctx.h)
            assert lib.dwgsim_hip_set_truth_depth(ctx.h, 0) == 0
    assert lib.dwgsim_hip_truth_vcf_header(None, None, 1, None, 0) == ERR_ARG and lib.dwgsim_hip_truth_vcf_header(None, None, 0, None, 0) > 0
    head = api.truth_vcf_header(contigs, lib).decode().split("\n")
    assert [l[:13] for l in head[-5:-2]] == ["##FORMAT=<ID=", "##FORMAT=<ID="[:13], "##FORMAT=<ID="] and [l.split(",")[0][13:] for l in head[-5:-2]] == ["GT", "AD", "DP"]
    assert "Number=1,Type=String" in head[-5] and "Number=.,Type=Integer" in head[-4] and "Number=1,Type=Integer" in head[-3]
    assert head[-2] == "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tdwgsim" and head[-1] == ""


# ---- 9. the job level and the command line ----
def check_levels(lib):
    contigs, flags = group_case()
    ctx_level = run_ctx(lib, flags, contigs, group_bp=0)
    check_result(lib, ctx_level, contigs, True, True)
    for kw in (dict(devices=[0]), dict(devices=[0, 0]), dict(devices=[0, 0, 0], gzip_on_gpu=True), dict(devices=[0], truth_sam=False)):
        kw.setdefault("gzip_on_gpu", False); kw.setdefault("truth_sam", True)
        job = api.run_job_api(api.parse_flags(flags, lib), contigs, batch_pairs=150, group_bp=6000, lib=lib, truth_vcf=True, **kw)
        assert job.truth_vcf == ctx_level.truth_vcf and job.truth_vcf_contigs == ["g1", "g2", "g3"] and job.truth_vcf_threads == 1, kw
        assert job.streams == ctx_level.streams and job.mutations_vcf == ctx_level.mutations_vcf and job.truth_sam == (ctx_level.truth_sam if kw["truth_sam"] else b""), kw
    plain = api.run_job_api(api.parse_flags(flags, lib), contigs, devices=[0], gzip_on_gpu=False, batch_pairs=150, group_bp=6000, lib=lib)
    assert plain.truth_vcf == b"" and plain.truth_vcf_contigs == [] and plain.streams == ctx_level.streams
    nomut = api.run_job_api(api.parse_flags(flags + " -M 1", lib), contigs, devices=[0, 0], gzip_on_gpu=False, batch_pairs=150, group_bp=6000, lib=lib, truth_vcf=True)
    assert nomut.truth_vcf == ctx_level.truth_vcf and nomut.mutations_txt == b""      # -M 1: no mutation files, the truth VCF all the same
    # the sink is refused once the job runs, and for reads the truth SAM is not made for
    import ctypes as C
    for f, want in (("-z 3 -N 10 -c 1", ERR_UNSUP), ("-z 3 -N 10 -c 2 -f TACG -2 0", ERR_UNSUP)):
        sink = api.JobSink(None, api.MUT_CB(), api.READS_CB(), api.MSG_CB(lambda u, m: None), api.READS_AT_CB())
        err = C.c_int(0)
        job = lib.dwgsim_hip_job_create(C.byref(api.parse_flags(f, lib)), None, 0, C.byref(sink), None, C.byref(err))
        assert job
        cb = api.TVCF_CB(lambda u, n, v, vl: 0)
        assert lib.dwgsim_hip_job_set_truth_vcf_sink(job, cb, None) == want and b"Illumina" in lib.dwgsim_hip_job_last_error(job)
        lib.dwgsim_hip_job_destroy(job)


def write_fasta(path, contigs):
    with open(path, "w") as f:
        for name, arr in contigs:
            s = bytes(bytearray(arr)).decode()
            f.write(f">{name}\n" + "".join(s[i:i + 70] + "\n" for i in range(0, len(s), 70)))


def check_cli(lib, cli, tmp_path, gzip_mode):
    contigs, flags = group_case()
    fa = os.path.join(str(tmp_path), "in.fa")
    write_fasta(fa, contigs)
    base = {k: v for k, v in os.environ.items() if not k.startswith("DWGSIM_HIP_TRUTH")}
    base.update(DWGSIM_HIP_GZIP=gzip_mode, DWGSIM_HIP_GROUP_BP="6000", DWGSIM_HIP_BATCH="150")
    outs = {}
    for tag, extra, more in (("on", {"DWGSIM_HIP_TRUTH_VCF": "1"}, ""), ("off", {}, ""), ("zero", {"DWGSIM_HIP_TRUTH_VCF": "0"}, ""), ("nomut", {"DWGSIM_HIP_TRUTH_VCF": "1"}, " -M 1")):
        prefix = os.path.join(str(tmp_path), tag)
        subprocess.run([cli] + (flags + more).split() + [fa, prefix], check=True, stderr=subprocess.DEVNULL, env=dict(base, **extra), timeout=600)
        outs[tag] = {name[len(tag):]: open(os.path.join(str(tmp_path), name), "rb").read() for name in sorted(os.listdir(str(tmp_path))) if name.startswith(tag + ".")}
    want = run_ctx(lib, flags, contigs, group_bp=0)
    assert outs["on"][".truth.vcf"] == api.truth_vcf_header(contigs, lib) + want.truth_vcf
    assert strip_truth_vcf(outs["on"][".truth.vcf"]) == outs["on"][".mutations.vcf"]
    assert len(outs["off"]) == 5 and ".truth.vcf" not in outs["off"] and outs["zero"] == outs["off"]
    assert {k: v for k, v in outs["on"].items() if k != ".truth.vcf"} == outs["off"]
    assert outs["nomut"][".truth.vcf"] == outs["on"][".truth.vcf"] and ".mutations.vcf" not in outs["nomut"]
    # refused with the message for SOLiD and Ion Torrent reads, and a failing job leaves no file
    for more in ("-c 1", "-c 2 -f TACG -2 0"):
        prefix = os.path.join(str(tmp_path), "refused")
        p = subprocess.run([cli] + f"-z 3 -N 10 {more}".split() + [fa, prefix], capture_output=True, env=dict(base, DWGSIM_HIP_TRUTH_VCF="1"), timeout=600)
        assert p.returncode != 0 and b"the truth VCF is made for Illumina reads only" in p.stderr and not os.path.exists(prefix + ".truth.vcf"), more
    bad = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "odd.fa")      # (the job the abort-rule tests give up on: tests/test_emu_parity.py)
    prefix = os.path.join(str(tmp_path), "failed")
    p = subprocess.run([cli] + "-z 6466 -1 33 -2 150 -d 900 -s 50 -N 1200 -r 0.01 -e 0.0-0.1 -Q 0 -a".split() + [bad, prefix], capture_output=True, env=dict(base, DWGSIM_HIP_TRUTH_VCF="1"), timeout=600)
    assert p.returncode != 0 and b"failed to generate a read" in p.stderr and not os.path.exists(prefix + ".truth.vcf") and os.path.exists(prefix + ".mutations.vcf")
