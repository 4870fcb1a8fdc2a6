"""The truth SAM (include/dwgsim_hip.h dwgsim_hip_set_truth_sam; DESIGN.md "6e"): a plain-Python checker and the cases tests/test_emu_truth_sam.py (CPU
emulation) and tests/test_gpu_truth_sam.py (device) both run.  Every check_* function takes the loaded library.

The checker does not replay the random numbers.  It holds every record to the FASTQ text of the same run (names, bases, qualities, order), to itself
(FLAG, mate fields, TLEN, CIGAR length) and to the job's own mutations.txt: walking the reference from POS along the CIGAR on haplotype HP, an M cell is not
deleted there, a D cell is, an I stands behind a cell that carries an insertion (all of it, or its first / last bases where the read stops inside it), no
indel cell of the span is missing, and -- error-free runs -- the bases this implies are SEQ."""
import gzip
import os
import re
import subprocess

import numpy as np

from dwgsim_amd import api
from hapfasta_common import edits_to_txt, normalise, parse_mutations_txt, revcomp, synth

ERR_ARG, ERR_UNSUP, ERR_STATE = -1, -4, -6
CIGAR_RE = re.compile(r"(\d+)([MID])")


def parse_cigar(c: str):
    ops = [(int(n), o) for n, o in CIGAR_RE.findall(c)]
    assert ops and "".join(f"{n}{o}" for n, o in ops) == c, c
    return ops


def hap_cells(edits, hap: int) -> dict:
    """{cell: (kind, bases)} of one haplotype (hap 0 / 1 = mask bit 1 / 2) from the edits of hapfasta_common"""
    return {pos: (kind, bases) for pos, kind, bases, mask in edits if mask & (1 << hap)}


def fastq_in_sam_order(streams):
    """[(name without '@' and '/1' '/2', seq, qual)] in the order of the truth SAM: pair by pair, end 1 then end 2.  From the BWA streams where they exist
    (-o 0, -o 1), else from the interleaved BFAST stream."""
    def recs(text, strip):
        lines = text.decode().split("\n")
        assert lines[-1] == "" and (len(lines) - 1) % 4 == 0
        out = []
        for k in range(0, len(lines) - 1, 4):
            name = lines[k]
            assert name[0] == "@" and lines[k + 2] == "+"
            if strip:
                assert name[-2:] in ("/1", "/2")
                name = name[:-2]
            out.append((name[1:], lines[k + 1], lines[k + 3]))
        return out
    if streams[api.STREAM_BWA1]:
        r1, r2 = recs(streams[api.STREAM_BWA1], True), recs(streams[api.STREAM_BWA2], True) if streams[api.STREAM_BWA2] else []
        if not r2:
            return r1
        assert len(r1) == len(r2)
        return [r for pair in zip(r1, r2) for r in pair]
    return recs(streams[api.STREAM_BFAST], False)


def name_fields(qname: str):
    """(contig with its prefix, pos1, pos2) of a read name <contig>_<pos1>_<pos2>_<s1>_<s2>_0_0_<e:s:i>_<e:s:i>_<hex>"""
    f = qname.rsplit("_", 9)
    assert len(f) == 10, qname
    return f[0], int(f[1]), int(f[2])


class Stats:
    def __init__(self):
        self.records = self.mapped = self.with_indel = self.rev_start_i = self.fwd_end_i = self.fwd_start_i = self.rev_end_i = self.hp = 0
        self.hap_seen = set()
        self.max_cigar_ops = 0


def check_alignment(rec, ref: str, cells: dict, exact: bool):
    """one mapped record against its haplotype; returns (lo, hi, has_indel): the 0-based span and whether the CIGAR holds an I or D"""
    pos0 = rec["pos"] - 1
    ops = parse_cigar(rec["cigar"])
    assert sum(n for n, o in ops if o in "MI") == len(rec["seq"]), rec["qname"]
    assert all(ops[k][1] != ops[k + 1][1] for k in range(len(ops) - 1)), "adjacent equal operations are merged"
    assert ops[0][1] != "D" and ops[-1][1] != "D" and any(o == "M" for _, o in ops)
    bases, c, last_m = [], pos0, None
    for k, (n, o) in enumerate(ops):
        if o == "I" and k == 0:
            # a reverse read that stopped inside an insertion: it belongs to the nearest cell left of POS that is not deleted, and holds its LAST n bases
            q = pos0 - 1
            while cells.get(q, ("", ""))[0] == "D":
                q -= 1
            kind, ins = cells.get(q, ("", ""))
            assert kind == "I" and n <= len(ins) and q >= 0, rec["qname"]
            bases.append(ins[len(ins) - n:])
        elif o == "I":
            kind, ins = cells.get(last_m, ("", ""))
            assert ops[k - 1][1] == "M" and kind == "I", rec["qname"]
            assert n == len(ins) if k + 1 < len(ops) else n <= len(ins), rec["qname"]      # fewer bases only at the read's end
            bases.append(ins[:n])
        elif o == "D":
            for q in range(c, c + n):
                assert cells.get(q, ("", ""))[0] == "D", (rec["qname"], q)
            c += n
        else:
            for q in range(c, c + n):
                assert 0 <= q < len(ref), rec["qname"]
                kind, b = cells.get(q, ("", ""))
                assert kind != "D", (rec["qname"], q)
                bases.append(b if kind == "S" else ref[q])
                if kind == "I":      # an insertion inside the span is in the CIGAR: the run ends here and an I follows, unless this is the alignment's last cell
                    last_of_all = q == c + n - 1 and all(o2 == "I" for _, o2 in ops[k + 1:])
                    assert q == c + n - 1 and (last_of_all or (k + 1 < len(ops) and ops[k + 1][1] == "I")), (rec["qname"], q)
            c += n
            last_m = c - 1
    if exact:
        assert "".join(bases) == rec["seq"], rec["qname"]
    return pos0, c - 1, len(ops) > 1


def check_sam(sam: bytes, streams, contigs, mutations_txt: bytes, paired: bool, exact: bool, prefix: str = "") -> Stats:
    """every record of a truth SAM against the FASTQ text and the mutations.txt of the same run"""
    fq = fastq_in_sam_order(streams)
    lines = sam.decode().split("\n")
    assert lines[-1] == "" and len(lines) - 1 == len(fq), (len(lines) - 1, len(fq))
    refs = {name: normalise(arr) for name, arr in contigs}
    edits = parse_mutations_txt(mutations_txt) if mutations_txt else {}
    cells = {(name, h): hap_cells(edits.get(name, []), h) for name in refs for h in (0, 1)}
    st = Stats()
    recs = []
    for line, (fname, fseq, fqual) in zip(lines, fq):
        f = line.split("\t")
        r = dict(qname=f[0], flag=int(f[1]), rname=f[2], pos=int(f[3]), mapq=int(f[4]), cigar=f[5], rnext=f[6], pnext=int(f[7]), tlen=int(f[8]), seq=f[9], qual=f[10])
        assert r["qname"] == fname, (r["qname"], fname)
        if prefix:
            assert fname.startswith(prefix + "_")
        unmapped = bool(r["flag"] & 4)
        assert len(f) == (11 if unmapped else 12), line
        if r["flag"] & 16:
            assert r["seq"] == revcomp(fseq) and r["qual"] == fqual[::-1], fname
        else:
            assert r["seq"] == fseq and r["qual"] == fqual, fname
        assert bool(r["flag"] & 1) == paired and r["flag"] & ~(1 | 2 | 4 | 8 | 16 | 32 | 64 | 128) == 0
        if unmapped:
            assert (r["rname"], r["pos"], r["mapq"], r["cigar"], r["rnext"], r["pnext"], r["tlen"]) == ("*", 0, 0, "*", "*", 0, 0), line
            assert r["flag"] & (2 | 16 | 32) == 0 and bool(r["flag"] & 8) == paired
            assert fname[len(prefix) + 1 if prefix else 0:].startswith("rand_"), fname
        else:
            assert f[11] in ("HP:i:1", "HP:i:2") and r["mapq"] == 60 and r["rname"] in refs, line
            r["hap"] = int(f[11][-1]) - 1
            contig, p1, p2 = name_fields(fname)
            assert contig == (prefix + "_" if prefix else "") + r["rname"], fname
            r["lo"], r["hi"], indel = check_alignment(r, refs[r["rname"]], cells[(r["rname"], r["hap"])], exact)
            st.mapped += 1; st.with_indel += indel; st.hap_seen.add(r["hap"])
            ops = parse_cigar(r["cigar"])
            st.max_cigar_ops = max(st.max_cigar_ops, len(ops))
            rev = bool(r["flag"] & 16)
            st.fwd_end_i += (not rev) and ops[-1][1] == "I"; st.rev_start_i += rev and ops[0][1] == "I"
            st.fwd_start_i += (not rev) and ops[0][1] == "I"; st.rev_end_i += rev and ops[-1][1] == "I"
            # the name's coordinate: a forward read's is its first cell; any read's, when no indel cell of its haplotype lies in the span (a leading I -- the
            # cell that carries it lies outside the span, and deleted cells may stand between -- is left out)
            second = bool(r["flag"] & 128)
            span_indel = any(k in ("I", "D") and r["lo"] <= q <= r["hi"] for q, (k, _) in cells[(r["rname"], r["hap"])].items())
            if (not rev and ops[0][1] != "I") or (not span_indel and ops[0][1] != "I"):
                assert r["pos"] == (p2 if second else p1), (fname, r["pos"], p1, p2)
        recs.append(r)
        st.records += 1
    if paired:
        assert len(recs) % 2 == 0
        for a, b in zip(recs[0::2], recs[1::2]):
            assert a["qname"] == b["qname"] and a["flag"] & 64 and b["flag"] & 128 and not a["flag"] & 128 and not b["flag"] & 64
            assert bool(a["flag"] & 4) == bool(b["flag"] & 4)
            if a["flag"] & 4:
                continue
            assert a["flag"] & 2 and b["flag"] & 2 and a["rname"] == b["rname"] and a["hap"] == b["hap"] and a["rnext"] == b["rnext"] == "="
            assert a["pnext"] == b["pos"] and b["pnext"] == a["pos"]
            assert bool(a["flag"] & 32) == bool(b["flag"] & 16) and bool(b["flag"] & 32) == bool(a["flag"] & 16)
            span = max(a["hi"], b["hi"]) - min(a["lo"], b["lo"]) + 1
            a_first = a["lo"] <= b["lo"]      # end 1 on a tie
            assert (a["tlen"], b["tlen"]) == ((span, -span) if a_first else (-span, span)), a["qname"]
    else:
        for r in recs:
            assert r["flag"] & ~(4 | 16) == 0 and (r["rnext"], r["pnext"], r["tlen"]) == ("*", 0, 0)
    return st


def run_ctx(lib, flags: str, contigs, **kw):
    res = api.run_job(api.parse_flags(flags, lib), contigs, lib=lib, truth_sam=True, **kw)
    return res


def check_run(lib, flags: str, contigs, exact: bool, prefix: str = "", **kw):
    p = api.parse_flags(flags, lib)
    res = run_ctx(lib, flags, contigs, **kw)
    st = check_sam(res.truth_sam, res.streams, contigs, res.mutations_txt, p.length[1] > 0, exact, prefix)
    plain = api.run_job(api.parse_flags(flags, lib), contigs, lib=lib, **kw)      # off: every other output is what it is without the feature
    assert plain.truth_sam == b"" and plain.streams == res.streams and plain.mutations_txt == res.mutations_txt
    return res, st


# ---- the model itself, on cases small enough to write out ----
def check_model():
    ref = "ACGTACGTAC"
    cells = {2: ("D", ""), 5: ("I", "TT"), 7: ("S", "A")}
    rec = dict(qname="x", pos=1, cigar="2M1D3M2I2M", seq="ACTACTTGA")
    assert check_alignment(rec, ref, cells, True) == (0, 7, True)
    rec = dict(qname="x", pos=7, cigar="1I2M", seq="TGA")          # a reverse read that stopped inside the insertion behind cell 5
    assert check_alignment(rec, ref, cells, True) == (6, 7, True)
    rec = dict(qname="x", pos=5, cigar="2M1I", seq="ACT")          # a forward read that stopped inside it
    assert check_alignment(rec, ref, cells, True) == (4, 5, True)
    for bad in ("2M1D3M2M", "3M3M", "2M1D3M1I2M", "2M1D6M"):         # the insertion is missing / cut short in mid-read, the deletion read through
        try:
            check_alignment(dict(qname="x", pos=1, cigar=bad, seq="A" * 9), ref, cells, False)
        except AssertionError:
            continue
        raise RuntimeError(f"the checker accepted {bad}")


# ---- 1. placed edits through -m ----
def placed_case():
    """Two contigs in one group.  cA: a 200-base insertion (reads of 50 bases start and end inside it), a deletion run, deletions on every second cell of a
    40-cell window (the CIGAR 1M1D1M1D ... of the bound), heterozygous indels, edits at the first and last cells; cB: substitutions at its first and last
    cells, a homozygous deletion run and an insertion.  The neighbours of every edit are pinned so that left-justification moves nothing -- and the
    checker reads the run's own mutations.txt, not this list."""
    a, b = synth(7, 9000), synth(8, 5000)
    pins_a = {0: "A", 8999: "G", 8998: "A", 999: "A", 1000: "C", 1999: "A", 2004: "C", 2999: "A", 3000: "T"}
    pins_a.update({q: "ACGT"[q & 3] for q in range(2000, 2004)})
    pins_a.update({q: "ACGT"[q & 3] for q in range(5990, 6050)})
    pins_b = {0: "C", 4999: "T", 2089: "A", 2100: "C", 3499: "A", 3500: "T"}
    pins_b.update({q: "ACGT"[q & 3] for q in range(2090, 2100)})
    for arr, pins in ((a, pins_a), (b, pins_b)):
        for q, ch in pins.items():
            arr[q] = ord(ch)
    big = "".join("ACGT"[(7 * q + q // 5) & 3] for q in range(199)) + "G"
    edits = {
        "cA": [(0, "S", "T", 3), (8999, "I", "TTC", 3), (1000, "I", big, 3), (3000, "I", "CCCCCCG", 2)]
              + [(q, "D", "", 1) for q in range(2000, 2005)]
              + [(q, "D", "", 3) for q in range(6000, 6040, 2)],
        "cB": [(0, "S", "G", 2), (4999, "S", "A", 3), (3500, "I", "GGC", 1)] + [(q, "D", "", 3) for q in range(2090, 2101)],
    }
    return [("cA", a), ("cB", b)], edits


def check_placed(lib, tmp_path):
    contigs, edits = placed_case()
    path = os.path.join(str(tmp_path), "placed.txt")
    with open(path, "w") as f:
        for name, arr in contigs:
            f.write(edits_to_txt(name, normalise(arr), edits[name]))
    res, st = check_run(lib, f"-z 5 -e 0 -E 0 -y 0 -N 4000 -1 50 -2 50 -m {path}", contigs, True, group_bp=1 << 30)
    got = parse_mutations_txt(res.mutations_txt)
    assert {n: sorted(e) for n, e in got.items()} == {n: sorted(e) for n, e in edits.items()}, "the walk moved a placed edit"
    assert st.mapped == 8000 and st.hap_seen == {0, 1}
    # reads stop inside the 200-base insertion on both strands: a forward read's CIGAR then ENDS with I, a reverse read's STARTS with I -- and never the
    # other way round (a read starts, in its own direction, at a cell that gives a base)
    assert st.fwd_end_i >= 1 and st.rev_start_i >= 1 and st.fwd_start_i == 0 and st.rev_end_i == 0, vars(st)
    assert st.max_cigar_ops >= 41      # 1M1D1M1D ... over the window of every second cell deleted (50 bases: at least 20 deletions inside)


# ---- 2. random walks ----
def check_random_walk(lib, errors: bool):
    contigs = [("walkA", synth(31, 10000)), ("walkB", synth(32, 9500))]
    flags = "-z 17 -r 0.02 -R 0.3 -X 0.5 -N 2000 -1 70 -2 70" + ("" if errors else " -e 0 -E 0")
    res, st = check_run(lib, flags, contigs, not errors, group_bp=1 << 30)
    assert st.records == 4000 and st.mapped > 3000
    assert st.with_indel >= 0.10 * st.mapped, (st.with_indel, st.mapped)


# ---- 3. the option surface ----
def surface_cases(tmp_path):
    bed = os.path.join(str(tmp_path), "two.bed")
    with open(bed, "w") as f:
        f.write("surf\t1000\t6000\nsurf\t9000\t15000\n")
    base = "-z 29 -r 0.01 -R 0.3 -X 0.4 -N 300"
    return [("single", base + " -2 0 -1 70", ""), ("random", base + " -y 0.1", ""), ("haploid", base + " -H", ""),
            ("S1", base + " -S 1", ""), ("S2", base + " -S 2", ""), ("A1", base + " -A 1", ""), ("A2", base + " -A 2", ""),
            ("inner", base + " -i", ""), ("regions", base + f" -x {bed}", ""), ("prefix", base + " -P pre", "pre"),
            ("o0", base + " -o 0", ""), ("o1", base + " -o 1", ""), ("o2", base + " -o 2", ""), ("o2single", base + " -o 2 -2 0", ""),
            ("r50", base + " -1 50 -2 50", ""), ("r70", base + " -1 70 -2 70", ""), ("r700", base + " -1 700 -2 700 -d 2000 -s 100", "")]


SURFACE_IDS = ["single", "random", "haploid", "S1", "S2", "A1", "A2", "inner", "regions", "prefix", "o0", "o1", "o2", "o2single", "r50", "r70", "r700", "amplicon"]


def check_surface(lib, tmp_path, which: str):
    contigs = [("surf", synth(41, 20000))]
    if which == "amplicon":
        contigs, flags, prefix = [("amp", synth(42, 199))], "-z 29 -r 0.02 -R 0.3 -N 200 -a -1 70 -2 70", ""      # (199 bases: synth puts no N into it; every read spans an amplicon end)
    else:
        _, flags, prefix = next(c for c in surface_cases(tmp_path) if c[0] == which)
    res, st = check_run(lib, flags, contigs, False, prefix)
    assert st.records in (200, 300, 400, 600) and st.mapped > 0
    # the k_simulate form the run took: reads of 50 bases the two-kernel form, 70 the single kernel, 700 the one-wave blocks
    forms = {api.unpack_sim_form(v) for v in res.sim_forms}
    if which in ("r50", "r70", "r700"):
        assert len(forms) == 1
        lpp, out, dt, nthr, wr, split = next(iter(forms))
        assert (dt, nthr, split) == {"r50": (0, 256, 1), "r70": (0, 256, 0), "r700": (0, 64, 0)}[which], forms
    if which == "random":
        assert st.mapped < st.records
    if which == "haploid":
        assert st.hap_seen <= {0, 1}


# ---- 4. batch shapes ----
def check_batch_shapes(lib):
    """1, 127, 128, 129 and 257 pairs per launch (one lane short of a block, a block, a lane more, two blocks and a lane), ranges that cross a contig boundary inside
    one launch, successive batches in different slots chained on the device: the records are those of one launch over everything"""
    contigs = [("sA", synth(51, 6000)), ("sB", synth(52, 7000))]
    flags = "-z 31 -r 0.01 -R 0.3 -N 514 -y 0.05"
    whole = run_ctx(lib, flags, contigs, group_bp=1 << 30)
    check_sam(whole.truth_sam, whole.streams, contigs, whole.mutations_txt, True, False)
    for bp in (1, 127, 128, 129, 257):
        if bp == 1:      # (a launch per pair: the first dozen pairs are enough)
            cut = api.run_job(api.parse_flags("-z 31 -r 0.01 -R 0.3 -N 12 -y 0.05", lib), contigs, lib=lib, truth_sam=True, group_bp=1 << 30, batch_pairs=1)
            one = api.run_job(api.parse_flags("-z 31 -r 0.01 -R 0.3 -N 12 -y 0.05", lib), contigs, lib=lib, truth_sam=True, group_bp=1 << 30)
            assert cut.truth_sam == one.truth_sam and cut.streams == one.streams and cut.truth_sam.count(b"\n") == 24
            continue
        cut = run_ctx(lib, flags, contigs, group_bp=1 << 30, batch_pairs=bp)
        assert cut.streams == whole.streams and cut.truth_sam == whole.truth_sam, bp
    # two slots, the second batch enqueued before the first was waited for, its random-read count chained on the device
    p = api.parse_flags(flags, lib)
    with api.Context(p, 0, lib) as ctx:
        ctx.set_truth_sam(True)
        sched = list(api.schedule_contigs(p, contigs, ctx, lib))
        h0 = ctx.add_contigs([(n, a) for _, n, a, _, _ in sched], indices=[ci for ci, _, _, _, _ in sched])
        ctx.mutate(h0)
        na, nb = sched[0][3], sched[1][3]
        ctx.simulate_ranges_async([(h0, 0, 100)], 0, 1)
        ctx.simulate_ranges_async([(h0, 100, na - 100), (h0 + 1, 0, nb)], api.RAND_CHAIN, 2)
        got = b""
        for slot in (1, 2):
            b = ctx.wait(slot)
            got += ctx.fetch(slot, api.STREAM_SAM, b.sam_bytes)
            assert ctx.count_byte(slot, api.STREAM_SAM, 10) == 2 * b.n_pairs
        assert got == whole.truth_sam


# ---- 5. levels ----
def levels_case():
    contigs = [("g1", synth(61, 6000)), ("tiny", synth(63, 100)), ("g2", synth(62, 9000)), ("g3", synth(64, 5000))]
    return contigs, "-z 23 -r 0.01 -R 0.2 -N 600 -1 60 -2 60"


def check_levels(lib):
    contigs, flags = levels_case()
    ctx_level = run_ctx(lib, flags, contigs, group_bp=0)
    st = check_sam(ctx_level.truth_sam, ctx_level.streams, contigs, ctx_level.mutations_txt, True, False)
    assert st.records == 1200
    for kw in (dict(gzip_on_gpu=False), dict(gzip_on_gpu=True), dict(gzip_on_gpu=False, offset_sink=True), dict(gzip_on_gpu=True, devices=[0, 0])):
        kw.setdefault("devices", [0])
        job = api.run_job_api(api.parse_flags(flags, lib), contigs, batch_pairs=150, group_bp=8000, lib=lib, truth_sam=True, **kw)
        assert job.truth_sam == ctx_level.truth_sam and job.streams == ctx_level.streams and job.mutations_txt == ctx_level.mutations_txt, kw
    plain = api.run_job_api(api.parse_flags(flags, lib), contigs, devices=[0], gzip_on_gpu=False, batch_pairs=150, group_bp=8000, lib=lib)
    assert plain.truth_sam == b"" and plain.streams == ctx_level.streams
    none = api.run_job_api(api.parse_flags(flags + " -M 2", lib), contigs, devices=[0], gzip_on_gpu=False, lib=lib, truth_sam=True)
    assert none.truth_sam == b""      # -M 2: no reads, no SAM
    # the members of stream 3 inflate to the text
    p = api.parse_flags(flags, lib)
    with api.Context(p, 0, lib) as ctx:
        ctx.set_truth_sam(True); ctx.set_gzip(True)
        h = ctx.add_contigs([contigs[0]])
        ctx.mutate(h)
        b = ctx.simulate(h, 0, 300, 0, 0)
        text = ctx.fetch(0, api.STREAM_SAM, b.sam_bytes)
        assert b.sam_bytes > 0 and b.sam_gz_bytes > 0 and b.sam_dev_ptr and text.count(b"\n") == 600
        assert gzip.decompress(ctx.fetch_gz(0, api.STREAM_SAM, b.sam_gz_bytes)) == text
    # the header: one exported function
    head = api.truth_sam_header(contigs, lib).decode().split("\n")
    assert head[0] == "@HD\tVN:1.6\tSO:unsorted\tGO:query" and head[1:5] == [f"@SQ\tSN:{n}\tLN:{len(a)}" for n, a in contigs] and head[5].startswith("@PG\t") and head[6:] == [""]


def check_cli(lib, cli, tmp_path, gzip_mode):
    contigs, flags = levels_case()
    fa = os.path.join(str(tmp_path), "in.fa")
    with open(fa, "w") as f:
        for name, arr in contigs:
            s = bytes(bytearray(arr)).decode()
            f.write(f">{name}\n" + "".join(s[i:i + 70] + "\n" for i in range(0, len(s), 70)))
    base = {k: v for k, v in os.environ.items() if not k.startswith("DWGSIM_HIP_TRUTH_SAM")}
    base.update(DWGSIM_HIP_GZIP=gzip_mode, DWGSIM_HIP_GROUP_BP="8000", DWGSIM_HIP_BATCH="150")
    outs = {}
    for tag, extra in (("on", {"DWGSIM_HIP_TRUTH_SAM": "1"}), ("off", {}), ("zero", {"DWGSIM_HIP_TRUTH_SAM": "0"}), ("empty", {"DWGSIM_HIP_TRUTH_SAM": ""})):
        prefix = os.path.join(str(tmp_path), tag)
        subprocess.run([cli] + flags.split() + [fa, prefix], check=True, stderr=subprocess.DEVNULL, env=dict(base, **extra), timeout=600)
        outs[tag] = {}
        for name in sorted(os.listdir(str(tmp_path))):
            if name.startswith(tag + "."):
                data = open(os.path.join(str(tmp_path), name), "rb").read()
                outs[tag][name[len(tag):]] = gzip.decompress(data) if name.endswith(".gz") else data
    want = run_ctx(lib, flags, contigs, group_bp=0)
    assert outs["on"][".truth.sam.gz"] == api.truth_sam_header(contigs, lib) + want.truth_sam
    assert len(outs["off"]) == 5 and ".truth.sam.gz" not in outs["off"] and outs["zero"] == outs["off"] and outs["empty"] == outs["off"]
    assert {k: v for k, v in outs["on"].items() if k != ".truth.sam.gz"} == outs["off"]


# ---- 6. errors ----
def check_errors(lib):
    import ctypes as C
    for flags in ("-z 3 -N 10 -c 1", "-z 3 -N 10 -c 2 -f TACG -2 0"):
        with api.Context(api.parse_flags(flags, lib), 0, lib) as ctx:
            assert lib.dwgsim_hip_set_truth_sam(ctx.h, 1) == ERR_UNSUP and lib.dwgsim_hip_last_error(ctx.h)
            assert lib.dwgsim_hip_set_truth_sam(ctx.h, 0) == 0
    p = api.parse_flags("-z 3 -r 0.01 -N 100", lib)
    with api.Context(p, 0, lib) as ctx:
        h = ctx.add_contigs([("e", synth(71, 5000))])
        ctx.mutate(h)
        buf = C.create_string_buffer(1 << 20)
        n = C.c_uint64(0)
        b = ctx.simulate(h, 0, 50, 0, 0)      # off: no SAM, and stream 3 is no stream
        assert b.sam_bytes == 0 and b.sam_gz_bytes == 0 and not b.sam_dev_ptr
        assert lib.dwgsim_hip_fetch(ctx.h, 0, api.STREAM_SAM, buf, 1 << 20) == ERR_ARG
        assert lib.dwgsim_hip_fetch_async(ctx.h, 0, api.STREAM_SAM, buf, 1 << 20) == ERR_ARG
        assert lib.dwgsim_hip_fetch_gz_async(ctx.h, 0, api.STREAM_SAM, buf, 1 << 20) == ERR_ARG
        assert lib.dwgsim_hip_debug_count_byte(ctx.h, 0, api.STREAM_SAM, 10, C.byref(n)) == ERR_ARG
        assert lib.dwgsim_hip_fetch(ctx.h, 0, 4, buf, 1 << 20) == ERR_ARG
        ctx.simulate_async(h, 0, 50, 0, 1)
        assert lib.dwgsim_hip_set_truth_sam(ctx.h, 1) == ERR_STATE      # a slot is pending
        ctx.wait(1)
        ctx.set_truth_sam(True)
        b = ctx.simulate(h, 0, 50, 0, 0)
        assert b.sam_bytes > 0 and ctx.fetch(0, api.STREAM_SAM, b.sam_bytes).count(b"\n") == 100
        ctx.set_truth_sam(False)
        assert lib.dwgsim_hip_fetch(ctx.h, 0, api.STREAM_SAM, buf, 1 << 20) == ERR_ARG
    assert lib.dwgsim_hip_truth_sam_header(None, None, 1, None, 0) == ERR_ARG and lib.dwgsim_hip_truth_sam_header(None, None, 0, None, 0) > 0
