"""The NM and MD tags of the truth SAM (include/dwgsim_hip.h dwgsim_hip_set_truth_md; DESIGN.md "6e"): a plain-Python checker and the cases that
tests/test_emu_truth_md.py (CPU emulation) and tests/test_gpu_truth_md.py (device) both run.  Every check_* function takes the loaded library.

NM and MD are pure functions of (reference, POS, CIGAR, SEQ), so the checker replays no random numbers and leaves no record out: every mapped record of every
case is held to the law computed forwards (expected_nm_md), to the law run backwards (the reference rebuilt from SEQ, CIGAR and MD alone, and NM counted from
MD and CIGAR), and -- the two tags cut off -- to the bytes of the same run without the switch."""
import gzip
import os
import re
import subprocess

import numpy as np

import truth_sam_common as T
from dwgsim_amd import api
from hapfasta_common import edits_to_txt, normalise, parse_mutations_txt, synth

ERR_UNSUP, ERR_STATE = T.ERR_UNSUP, T.ERR_STATE
MD_RE = re.compile(r"[0-9]+(([A-Z]|\^[A-Z]+)[0-9]+)*")
MD_TOK = re.compile(r"([0-9]+)|\^([A-Z]+)|([A-Z])")


# ---- the law, forwards ----
def walk_law(ref: str, pos: int, cigar: str, seq: str):
    """(NM, MD, the 0-based cells of the mismatches) of a record: `ref` the contig as upper-case ACGT / N, pos 1-based, seq as the SAM line prints it"""
    c, q, nm, run, out, mism = pos - 1, 0, 0, 0, [], []
    for n, o in T.parse_cigar(cigar):
        if o == "I":
            nm += n; q += n
        elif o == "D":
            out.append(f"{run}^{ref[c:c + n]}"); run = 0; nm += n; c += n
        else:
            for _ in range(n):
                r, b = ref[c], seq[q]
                if b == r and r in "ACGT":
                    run += 1
                else:
                    out.append(f"{run}{r}"); run = 0; nm += 1; mism.append(c)
                c += 1; q += 1
    assert q == len(seq)
    out.append(str(run))
    return nm, "".join(out), mism


def expected_nm_md(ref: str, pos: int, cigar: str, seq: str):
    nm, md, _ = walk_law(ref, pos, cigar, seq)
    return nm, md


# ---- the law, backwards: nothing here looks at the reference ----
def rebuild_reference(cigar: str, seq: str, md: str):
    """(the reference over the alignment's span, NM) from SEQ, CIGAR and MD alone"""
    assert MD_RE.fullmatch(md), md
    cells = []      # one entry per reference cell of the span, in order: "=" a match, ("X", r) a mismatch, ("D", letters) a whole deletion run
    for num, dele, letter in MD_TOK.findall(md):
        if num:
            assert num == str(int(num)), f"a count with leading zeros in {md}"
            cells.extend("=" * int(num))
        elif dele:
            cells.append(("D", dele))
        else:
            cells.append(("X", letter))
    out, k, q, n_x, n_d, n_i = [], 0, 0, 0, 0, 0
    for n, o in T.parse_cigar(cigar):
        if o == "I":
            q += n; n_i += n
        elif o == "D":
            assert k < len(cells) and cells[k][0] == "D" and len(cells[k][1]) == n, f"{cigar} / {md}: the deletion run of {n}"
            out.append(cells[k][1]); k += 1; n_d += n
        else:
            for _ in range(n):
                assert k < len(cells) and cells[k][0] != "D", f"{cigar} / {md}: an M cell where MD holds a deletion or nothing"
                if cells[k] == "=":
                    assert seq[q] in "ACGT", "only A C G T match"
                    out.append(seq[q])
                else:
                    r = cells[k][1]
                    assert r != seq[q] or r == "N", f"{md}: a mismatch that names the read's own base"
                    out.append(r); n_x += 1
                k += 1; q += 1
    assert k == len(cells) and q == len(seq), f"{cigar} / {md}: MD and CIGAR cover different spans"
    return "".join(out), n_x + n_d + n_i


def check_tags(ref: str, pos: int, cigar: str, seq: str, nm_field: str, md_field: str):
    """the two fields of one mapped record against the law, both ways; returns (NM, MD, mismatch cells)"""
    assert nm_field.startswith("NM:i:") and md_field.startswith("MD:Z:"), (nm_field, md_field)
    nm_txt, md = nm_field[5:], md_field[5:]
    assert nm_txt.isdigit() and nm_txt == str(int(nm_txt)), nm_field
    want_nm, want_md, mism = walk_law(ref, pos, cigar, seq)
    assert (int(nm_txt), md) == (want_nm, want_md), (pos, cigar, seq, nm_field, md_field, want_nm, want_md)
    span, nm_back = rebuild_reference(cigar, seq, md)
    assert span == ref[pos - 1:pos - 1 + len(span)], (pos, cigar, md)
    letters_out = sum(1 for _, d, x in MD_TOK.findall(md) if x)
    letters_in = sum(len(d) for _, d, x in MD_TOK.findall(md))
    assert int(nm_txt) == nm_back == letters_out + letters_in + sum(n for n, o in T.parse_cigar(cigar) if o == "I"), (nm_field, md_field, cigar)
    return want_nm, want_md, mism


def check_model():
    """hand-written records the checker accepts, and wrong ones it rejects"""
    good = [
        ("ACGTACGTAC" + "AC" + "T" + "GGGGG", 1, "10M2D6M", "ACGTACGTAC" + "A" + "GGGGG", 3, "10^AC0T5"),      # a mismatch directly behind a deletion gets its 0
        ("ACGTACGT", 3, "2I4M3I", "TT" + "GTAC" + "CCC", 5, "4"),                                              # a leading and a trailing I: NM counts them, MD does not see them
        ("ACGTACGT", 3, "2M2I2M", "GT" + "GG" + "AC", 2, "4"),                                                 # ... nor does an I inside interrupt the count
        ("ACNNGT", 1, "6M", "ACNNGT", 2, "2N0N2"),                                                             # N on N is a mismatch
        ("ACGTA", 1, "5M", "ACGTA", 0, "5"),                                                                   # a cell substituted on the haplotype, put back to the reference base by an error: a match
        ("ACGTA", 1, "5M", "TCGTC", 2, "0A3A0"),                                                               # the first and the last cell: the counts at both ends stand, also as 0
        ("ACGTACGTAC", 2, "3M4D2M", "CGTAC", 4, "3^ACGT2"),
    ]
    for ref, pos, cigar, seq, nm, md in good:
        assert expected_nm_md(ref, pos, cigar, seq) == (nm, md), (cigar, expected_nm_md(ref, pos, cigar, seq))
        check_tags(ref, pos, cigar, seq, f"NM:i:{nm}", f"MD:Z:{md}")
    ref, pos, cigar, seq = good[0][:4]
    bad = [("NM:i:3", "MD:Z:10^ACT5"), ("NM:i:3", "MD:Z:10^ac0t5"), ("NM:i:3", "MD:Z:10AC0T5"), ("NM:i:4", "MD:Z:10^AC0T5"), ("NM:i:2", "MD:Z:10^AC0T5"),
           ("NM:i:03", "MD:Z:10^AC0T5"), ("NM:i:3", "MD:Z:10^AC0T05"), ("NM:i:3", "MD:Z:10^AC0T"), ("NM:i:3", "MD:Z:^AC0T5"), ("nm:i:3", "MD:Z:10^AC0T5")]
    for nm_f, md_f in bad:      # a missing 0, lower case, a deletion without ^, NM off by one either way, leading zeros, no count at an end, a wrong tag name
        try:
            check_tags(ref, pos, cigar, seq, nm_f, md_f)
        except AssertionError:
            continue
        raise RuntimeError(f"the checker accepted {nm_f} {md_f}")
    # ... and the backwards half rejects on its own what does not fit the CIGAR or names the read's base
    for cg, sq, md in (("10M2D6M", seq, "10^ACT5"), ("10M2D6M", seq, "10AC0T5"), ("5M", "ACGTA", "2G2"), ("5M", "ACGTA", "4"), ("5M", "ACNTA", "5")):
        try:
            rebuild_reference(cg, sq, md)
        except AssertionError:
            continue
        raise RuntimeError(f"the backwards check accepted {cg} {md}")


# ---- a tagged truth SAM against the untagged one of the same run ----
class Stats:
    def __init__(self):
        self.records = self.mapped = self.nm0 = self.fwd = self.rev = self.err_mismatch = self.sub_mismatch = self.md_n = self.del0 = 0
        self.fwd_end_i = self.rev_start_i = self.comb = 0
        self.hap_seen = set()
        self.mds = []

    def summary(self):
        return {k: v for k, v in vars(self).items() if k != "mds"}


def check_tagged(tagged: bytes, plain: bytes, contigs, mutations_txt: bytes) -> Stats:
    """every record: unmapped ones are the untagged line; mapped ones are it with fields 13-14 behind, and those are the law's"""
    refs = {name: normalise(arr) for name, arr in contigs}
    edits = parse_mutations_txt(mutations_txt) if mutations_txt else {}
    subs = {(name, h): {q for q, (k, _) in T.hap_cells(edits.get(name, []), h).items() if k == "S"} for name in refs for h in (0, 1)}
    a, b = tagged.decode().split("\n"), plain.decode().split("\n")
    assert a[-1] == "" and b[-1] == "" and len(a) == len(b), (len(a), len(b))
    st = Stats()
    for line, want in zip(a[:-1], b[:-1]):
        f = line.split("\t")
        st.records += 1
        if int(f[1]) & 4:
            assert line == want and len(f) == 11, line
            continue
        assert len(f) == 14 and "\t".join(f[:12]) == want, line
        hap = int(f[11][-1]) - 1
        nm, md, mism = check_tags(refs[f[2]], int(f[3]), f[5], f[9], f[12], f[13])
        st.mapped += 1; st.nm0 += nm == 0; st.hap_seen.add(hap)
        rev = bool(int(f[1]) & 16)
        st.rev += rev; st.fwd += not rev
        ops = T.parse_cigar(f[5])
        st.fwd_end_i += (not rev) and ops[-1][1] == "I"; st.rev_start_i += rev and ops[0][1] == "I"
        st.err_mismatch += any(q not in subs[(f[2], hap)] for q in mism); st.sub_mismatch += any(q in subs[(f[2], hap)] for q in mism)
        st.md_n += "N" in md; st.del0 += bool(re.search(r"\^[A-Z]+0[A-Z]", md)); st.comb += bool(re.search(r"([0-9]\^[A-Z]){10}", md))
        st.mds.append(md)
    return st


def run_pair(lib, flags: str, contigs, level=api.run_job, **kw):
    """the run with the tags and the same run without: (tagged result, untagged result, Stats).  Everything but the SAM is the same bytes."""
    tagged = level(api.parse_flags(flags, lib), contigs, lib=lib, truth_sam=True, truth_md=True, **kw)
    plain = level(api.parse_flags(flags, lib), contigs, lib=lib, truth_sam=True, **kw)
    assert tagged.streams == plain.streams and tagged.mutations_txt == plain.mutations_txt and tagged.mutations_vcf == plain.mutations_vcf
    return tagged, plain, check_tagged(tagged.truth_sam, plain.truth_sam, contigs, tagged.mutations_txt)


# ---- 1. placed edits through -m ----
def placed_case():
    """T.placed_case() and, on cA, a deletion directly followed by a substituted cell (^CG0T); the neighbours are pinned so that left-justification moves nothing"""
    contigs, edits = T.placed_case()
    a = contigs[0][1]
    for q, ch in {3999: "A", 4000: "C", 4001: "G", 4002: "T", 4003: "C"}.items():
        a[q] = ord(ch)
    edits["cA"] = edits["cA"] + [(4000, "D", "", 3), (4001, "D", "", 3), (4002, "S", "A", 3)]
    return contigs, edits


def check_placed(lib, tmp_path):
    contigs, edits = placed_case()
    path = os.path.join(str(tmp_path), "placed.txt")
    with open(path, "w") as f:
        for name, arr in contigs:
            f.write(edits_to_txt(name, normalise(arr), edits[name]))
    tagged, plain, st = run_pair(lib, f"-z 5 -e 0 -E 0 -y 0 -N 4000 -1 50 -2 50 -m {path}", contigs, group_bp=1 << 30)
    got = parse_mutations_txt(tagged.mutations_txt)
    assert {n: sorted(e) for n, e in got.items()} == {n: sorted(e) for n, e in edits.items()}, "the walk moved a placed edit"
    assert st.mapped == 8000 and st.hap_seen == {0, 1} and st.fwd and st.rev
    assert st.fwd_end_i >= 1 and st.rev_start_i >= 1, st.summary()      # the 200-base insertion: a trailing I on forward reads, a leading one on reverse reads
    assert st.comb >= 1, "no read over the window of every second cell deleted (1^A1^C ...)"
    assert any("^CG0T" in md for md in st.mds), "no read over the deletion directly followed by a substituted cell"
    assert st.err_mismatch == 0 and st.sub_mismatch >= 1      # error-free: every mismatch is a substituted cell of the read's haplotype


# ---- 2. a reference with N and '-' ----
def check_ref_n(lib):
    rng = np.random.default_rng(91)
    a = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 3000)].copy()
    a[1000:1005] = ord("N"); a[2000] = ord("-"); a[2500:2503] = ord("n")
    tagged, plain, st = run_pair(lib, "-z 19 -r 0.005 -y 0 -N 600 -1 50 -2 50 -n 8 -d 200 -s 20", [("withN", a)])
    assert st.mapped == 1200 and st.md_n >= 3, st.summary()      # reads cross the runs: MD shows N there and NM counts those cells (check_tags, every record)
    assert any("N0N0N0N0N" in md for md in st.mds), "no read over the whole run of five N"


# ---- 3. random walks ----
def check_random_walk(lib, errors: bool):
    contigs = [("walkA", synth(31, 10000)), ("walkB", synth(32, 9500))]
    flags = "-z 17 -r 0.02 -R 0.3 -X 0.5 -N 2000 -1 70 -2 70" + ("" if errors else " -e 0 -E 0")
    tagged, plain, st = run_pair(lib, flags, contigs, group_bp=1 << 30)
    assert st.records == 4000 and st.mapped > 3000 and st.hap_seen == {0, 1} and st.fwd > 0 and st.rev > 0
    assert st.nm0 >= 1 and st.sub_mismatch >= 1
    if errors:
        assert st.err_mismatch >= 1, "no sequencing error showed in MD"
    else:
        assert st.err_mismatch == 0, "a mismatch that is no substituted cell of the read's haplotype in an error-free run"


# ---- 4. the option surface ----
SURFACE_IDS = ["single", "random", "haploid", "S2", "regions", "prefix", "o0", "o1", "o2", "o2single", "r50", "r70", "r700"]


def check_surface(lib, tmp_path, which: str):
    contigs = [("surf", synth(41, 20000))]
    _, flags, prefix = next(c for c in T.surface_cases(tmp_path) if c[0] == which)
    tagged, plain, st = run_pair(lib, flags, contigs)
    assert st.records in (300, 600) and st.mapped > 0
    forms = {api.unpack_sim_form(v) for v in tagged.sim_forms}
    if which in ("r50", "r70", "r700"):      # the two-kernel form, the single kernel, the one-wave blocks
        assert len(forms) == 1
        lpp, out, dt, nthr, wr, split = next(iter(forms))
        assert (dt, nthr, split) == {"r50": (0, 256, 1), "r70": (0, 256, 0), "r700": (0, 64, 0)}[which], forms
    if which == "random":
        assert st.mapped < st.records      # (random reads: untagged, the untagged run's line -- check_tagged)


# ---- 5. batch shapes ----
SHAPE_FLAGS = "-z 31 -r 0.01 -R 0.3 -N 514 -y 0.05"


def shape_contigs():
    return [("sA", synth(51, 6000)), ("sB", synth(52, 7000))]


def check_batch_shapes(lib):
    contigs = shape_contigs()
    whole, plain, st = run_pair(lib, SHAPE_FLAGS, contigs, group_bp=1 << 30)
    assert st.records == 1028
    for bp in (1, 127, 128, 129, 257):
        if bp == 1:      # (a launch per pair: the first dozen pairs are enough)
            small = "-z 31 -r 0.01 -R 0.3 -N 12 -y 0.05"
            cut = api.run_job(api.parse_flags(small, lib), contigs, lib=lib, truth_sam=True, truth_md=True, group_bp=1 << 30, batch_pairs=1)
            one = api.run_job(api.parse_flags(small, lib), contigs, lib=lib, truth_sam=True, truth_md=True, group_bp=1 << 30)
            assert cut.truth_sam == one.truth_sam and cut.streams == one.streams and cut.truth_sam.count(b"\n") == 24
            continue
        cut = api.run_job(api.parse_flags(SHAPE_FLAGS, lib), contigs, lib=lib, truth_sam=True, truth_md=True, group_bp=1 << 30, batch_pairs=bp)      # (ranges cross the contig boundary)
        assert cut.streams == whole.streams and cut.truth_sam == whole.truth_sam, bp
    got = two_slots(lib, None)
    assert b"".join(g["sam"] for g in got["batches"]) == whole.truth_sam and got["reruns"] == 0


def two_slots(lib, force, in_turn=False, cap=3000):
    """two batches in two slots, the second enqueued before the first was waited for (in_turn: only after it, so after its second run where it takes one), its
    random-read count chained on the device.  force: None, "both" or "first": which of them are planned with a truth_cap far too small"""
    contigs = shape_contigs()
    p = api.parse_flags(SHAPE_FLAGS, lib)
    with api.Context(p, 0, lib) as ctx:
        ctx.set_truth_sam(True); ctx.set_truth_md(True)
        sched = list(api.schedule_contigs(p, contigs, ctx, lib))
        h0 = ctx.add_contigs([(n, a) for _, n, a, _, _ in sched], indices=[ci for ci, _, _, _, _ in sched])
        ctx.mutate(h0)
        na, nb = sched[0][3], sched[1][3]
        if force:
            ctx.debug_option("truth_cap", cap)
        ctx.simulate_ranges_async([(h0, 0, 100)], 0, 1)
        first = ctx.wait(1) if in_turn else None
        reruns_first = ctx.debug_get("truth_reruns")
        if force == "first":
            ctx.debug_option("truth_cap", -1)
        ctx.simulate_ranges_async([(h0, 100, na - 100), (h0 + 1, 0, nb)], api.RAND_CHAIN, 2)
        out = []
        for slot in (1, 2):
            b = first if in_turn and slot == 1 else ctx.wait(slot)
            out.append(dict(n_pairs=b.n_pairs, n_random=b.n_random, n_retries=b.n_retries, fail_seg=tuple(b.fail_seg), fail_carry=b.fail_carry,
                            fastq=[ctx.fetch(slot, s, b.bytes[s]) for s in range(3)], sam=ctx.fetch(slot, api.STREAM_SAM, b.sam_bytes)))
            assert ctx.count_byte(slot, api.STREAM_SAM, 10) == 2 * b.n_pairs
        return dict(batches=out, reruns=ctx.debug_get("truth_reruns"), reruns_first=reruns_first)


# ---- 6. the second run ----
def check_second_run_forced(lib):
    contigs = shape_contigs()
    whole = api.run_job(api.parse_flags(SHAPE_FLAGS, lib), contigs, lib=lib, truth_sam=True, truth_md=True, group_bp=1 << 30)
    assert whole.truth_reruns == 0
    for bp in (1 << 22, 200):      # one batch; three batches of one context, each of them run twice
        forced = api.run_job(api.parse_flags(SHAPE_FLAGS, lib), contigs, lib=lib, truth_sam=True, truth_md=True, group_bp=1 << 30, batch_pairs=bp, debug_options={"truth_cap": 4096})
        assert forced.truth_sam == whole.truth_sam and forced.streams == whole.streams and forced.mutations_txt == whole.mutations_txt
        assert forced.truth_reruns >= (1 if bp > 514 else 3) and (forced.n_random, forced.n_retries, forced.n_pairs) == (whole.n_random, whole.n_retries, whole.n_pairs)
    # the batch itself and the next batch of the same context: counters, abort-rule words, FASTQ and SAM are those of the unforced run
    base = two_slots(lib, None)
    for force, reruns in (("both", 2), ("first", 1)):
        got = two_slots(lib, force)
        assert got["batches"] == base["batches"] and got["reruns"] == reruns, force
    # the tags off: "truth_cap" forces nothing, and no second run happens
    off = api.run_job(api.parse_flags(SHAPE_FLAGS, lib), contigs, lib=lib, truth_sam=True, group_bp=1 << 30, debug_options={"truth_cap": 4096})
    assert off.truth_reruns == 0 and off.truth_sam == api.run_job(api.parse_flags(SHAPE_FLAGS, lib), contigs, lib=lib, truth_sam=True, group_bp=1 << 30).truth_sam


def check_second_run_leaves_no_trace(lib):
    """a batch that takes the second run, and only then a batch on the other slot of the same context without the forced cap: the room the first one's scan asked
    for is its own.  The later batch is the larger one, so planned with that room it would run twice as well; planned as usual it runs once, and both batches
    are those of a context that never ran anything again"""
    base = two_slots(lib, None, in_turn=True)
    got = two_slots(lib, "first", in_turn=True, cap=4096)
    assert base["reruns_first"] == 0 and base["reruns"] == 0
    assert got["reruns_first"] == 1 and got["reruns"] == 1
    assert len(got["batches"][1]["sam"]) > len(got["batches"][0]["sam"]) > 4096
    assert got["batches"] == base["batches"] == two_slots(lib, None)["batches"]


def check_second_run_gzip(lib):
    """the second run with the gzip kernel behind the truth step (the default of the job level and of dwgsim-hip): the first run's gzip must take nothing of a SAM
    that did not fit, and the members of the second run inflate to the unforced text"""
    contigs = shape_contigs()
    whole = api.run_job(api.parse_flags(SHAPE_FLAGS, lib), contigs, lib=lib, truth_sam=True, truth_md=True, group_bp=1 << 30)
    p = api.parse_flags(SHAPE_FLAGS, lib)
    with api.Context(p, 0, lib) as ctx:
        ctx.set_truth_sam(True); ctx.set_truth_md(True); ctx.set_gzip(True)
        ctx.debug_option("truth_cap", 4096)
        sched = list(api.schedule_contigs(p, contigs, ctx, lib))
        h0 = ctx.add_contigs([(n, a) for _, n, a, _, _ in sched], indices=[ci for ci, _, _, _, _ in sched])
        ctx.mutate(h0)
        b = ctx.simulate_ranges([(h0, 0, sched[0][3]), (h0 + 1, 0, sched[1][3])], 0, 0)
        text = ctx.fetch(0, api.STREAM_SAM, b.sam_bytes)
        assert text == whole.truth_sam and gzip.decompress(ctx.fetch_gz(0, api.STREAM_SAM, b.sam_gz_bytes)) == text and ctx.debug_get("truth_reruns") == 1
        for s in range(2):
            assert gzip.decompress(ctx.fetch_gz(0, s, b.gz_bytes[s])) == whole.streams[s]
    for kw in (dict(devices=[0]), dict(devices=[0, 0]), dict(devices=[0], offset_sink=True)):
        job = api.run_job_api(api.parse_flags(SHAPE_FLAGS, lib), contigs, gzip_on_gpu=True, batch_pairs=150, group_bp=8000, lib=lib, truth_sam=True, truth_md=True,
                              debug_options={"truth_cap": 4096}, **kw)
        assert job.truth_sam == whole.truth_sam and job.streams == whole.streams and job.mutations_txt == whole.mutations_txt, kw
        assert job.truth_reruns >= 1, kw
    plain = api.run_job_api(api.parse_flags(SHAPE_FLAGS, lib), contigs, devices=[0], gzip_on_gpu=True, batch_pairs=150, group_bp=8000, lib=lib, truth_sam=True, truth_md=True)
    assert plain.truth_reruns == 0 and plain.truth_sam == whole.truth_sam


def natural_case():
    """a contig that is mostly deleted on both haplotypes: islands of 8 cells between deletions of 392, so that a single-end read of 50 bases spells out a
    few thousand deleted bases in its MD -- more than the slack of the planned buffer holds"""
    n = 4400
    rng = np.random.default_rng(77)
    a = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].copy()
    edits = [(q, "D", "", 3) for q in range(n) if 8 <= q % 400 and 200 <= q < n - 200]
    return [("holes", a)], {"holes": edits}


def check_second_run_natural(lib, tmp_path):
    contigs, edits = natural_case()
    path = os.path.join(str(tmp_path), "holes.txt")
    with open(path, "w") as f:
        f.write(edits_to_txt("holes", normalise(contigs[0][1]), edits["holes"]))
    flags = f"-z 9 -y 0 -N 400 -1 50 -2 0 -m {path}"
    tagged, plain, st = run_pair(lib, flags, contigs)
    assert tagged.truth_reruns >= 1, "the planned capacity held: the natural second run was not exercised"
    roomy = api.run_job(api.parse_flags(flags, lib), contigs, lib=lib, truth_sam=True, truth_md=True, debug_options={"truth_cap": 64 << 20})
    assert roomy.truth_reruns == 0 and roomy.truth_sam == tagged.truth_sam and roomy.streams == tagged.streams
    assert (roomy.n_random, roomy.n_retries) == (tagged.n_random, tagged.n_retries) == (plain.n_random, plain.n_retries)


# ---- 7. levels ----
def check_levels(lib):
    contigs, flags = T.levels_case()
    ctx_level, plain, st = run_pair(lib, flags, contigs, group_bp=0)
    assert st.records == 1200
    for kw in (dict(gzip_on_gpu=False), dict(gzip_on_gpu=True), dict(gzip_on_gpu=False, offset_sink=True), dict(gzip_on_gpu=True, devices=[0, 0])):
        kw.setdefault("devices", [0])
        job = api.run_job_api(api.parse_flags(flags, lib), contigs, batch_pairs=150, group_bp=8000, lib=lib, truth_sam=True, truth_md=True, **kw)
        assert job.truth_sam == ctx_level.truth_sam and job.streams == ctx_level.streams and job.mutations_txt == ctx_level.mutations_txt, kw
    alone = api.run_job_api(api.parse_flags(flags, lib), contigs, devices=[0], gzip_on_gpu=False, batch_pairs=150, group_bp=8000, lib=lib, truth_md=True)
    assert alone.truth_sam == b"" and alone.streams == ctx_level.streams      # on its own the switch produces no stream


def check_cli(lib, cli, tmp_path, gzip_mode):
    contigs, flags = T.levels_case()
    fa = os.path.join(str(tmp_path), "in.fa")
    with open(fa, "w") as f:
        for name, arr in contigs:
            s = bytes(bytearray(arr)).decode()
            f.write(f">{name}\n" + "".join(s[i:i + 70] + "\n" for i in range(0, len(s), 70)))
    base = {k: v for k, v in os.environ.items() if not k.startswith("DWGSIM_HIP_TRUTH_")}
    base.update(DWGSIM_HIP_GZIP=gzip_mode, DWGSIM_HIP_GROUP_BP="8000", DWGSIM_HIP_BATCH="150")
    outs = {}
    for tag, extra in (("both", {"DWGSIM_HIP_TRUTH_SAM": "1", "DWGSIM_HIP_TRUTH_MD": "1"}), ("alone", {"DWGSIM_HIP_TRUTH_MD": "1"}), ("off", {}),
                       ("zero", {"DWGSIM_HIP_TRUTH_SAM": "1", "DWGSIM_HIP_TRUTH_MD": "0"}), ("empty", {"DWGSIM_HIP_TRUTH_SAM": "1", "DWGSIM_HIP_TRUTH_MD": ""}), ("sam", {"DWGSIM_HIP_TRUTH_SAM": "1"})):
        prefix = os.path.join(str(tmp_path), tag)
        subprocess.run([cli] + flags.split() + [fa, prefix], check=True, stderr=subprocess.DEVNULL, env=dict(base, **extra), timeout=600)
        outs[tag] = {}
        for name in sorted(os.listdir(str(tmp_path))):
            if name.startswith(tag + "."):
                data = open(os.path.join(str(tmp_path), name), "rb").read()
                outs[tag][name[len(tag):]] = gzip.decompress(data) if name.endswith(".gz") else data
    # the second run through the program: a first capacity far too small (DWGSIM_HIP_DEBUG), the same files
    both_env = dict(base, DWGSIM_HIP_TRUTH_SAM="1", DWGSIM_HIP_TRUTH_MD="1")
    r = subprocess.run([cli] + flags.split() + [fa, os.path.join(str(tmp_path), "forced")], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, env=dict(both_env, DWGSIM_HIP_DEBUG="truth_cap=4096"), timeout=600)
    reruns = re.search(rb"\[dwgsim-hip-debug\] truth_reruns=(\d+)", r.stderr)
    assert reruns and int(reruns.group(1)) >= 1, r.stderr[-500:]
    forced = {}
    for name in sorted(os.listdir(str(tmp_path))):
        if name.startswith("forced."):
            data = open(os.path.join(str(tmp_path), name), "rb").read()
            forced[name[len("forced"):]] = gzip.decompress(data) if name.endswith(".gz") else data
    assert forced == outs["both"]
    r = subprocess.run([cli] + flags.split() + [fa, os.path.join(str(tmp_path), "unforced")], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, env=dict(both_env, DWGSIM_HIP_DEBUG="truth_cap=-1"), timeout=600)
    assert b"truth_reruns=0" in r.stderr
    want = api.run_job(api.parse_flags(flags, lib), contigs, lib=lib, truth_sam=True, truth_md=True, group_bp=0)
    assert outs["both"][".truth.sam.gz"] == api.truth_sam_header(contigs, lib) + want.truth_sam and b"\tMD:Z:" in want.truth_sam
    assert len(outs["off"]) == 5 and outs["alone"] == outs["off"]      # DWGSIM_HIP_TRUTH_MD alone: the five usual files and nothing else
    assert outs["zero"] == outs["sam"] and outs["empty"] == outs["sam"] and b"MD:Z:" not in outs["sam"][".truth.sam.gz"]
    assert {k: v for k, v in outs["both"].items() if k != ".truth.sam.gz"} == outs["off"]


# ---- 8. errors ----
def check_errors(lib):
    for flags in ("-z 3 -N 10 -c 1", "-z 3 -N 10 -c 2 -f TACG -2 0"):
        with api.Context(api.parse_flags(flags, lib), 0, lib) as ctx:
            assert lib.dwgsim_hip_set_truth_md(ctx.h, 1) == ERR_UNSUP and lib.dwgsim_hip_last_error(ctx.h)
            assert lib.dwgsim_hip_set_truth_md(ctx.h, 0) == 0
        try:
            api.run_job_api(api.parse_flags(flags, lib), [("e", synth(71, 5000))], devices=[0], gzip_on_gpu=False, lib=lib, truth_md=True)
        except api.DwgsimError as e:
            assert f"error {ERR_UNSUP}" in str(e)
        else:
            raise AssertionError("the job level took the switch for " + flags)
    p = api.parse_flags("-z 3 -r 0.01 -y 0 -N 100", lib)
    with api.Context(p, 0, lib) as ctx:
        h = ctx.add_contigs([("e", synth(71, 5000))])
        ctx.mutate(h)
        ctx.set_truth_md(True)      # the truth SAM is off: no stream 3
        b = ctx.simulate(h, 0, 50, 0, 0)
        assert b.sam_bytes == 0 and b.sam_gz_bytes == 0 and not b.sam_dev_ptr
        import ctypes as C
        buf = C.create_string_buffer(1 << 16)
        assert lib.dwgsim_hip_fetch(ctx.h, 0, api.STREAM_SAM, buf, 1 << 16) == T.ERR_ARG
        ctx.simulate_async(h, 0, 50, 0, 1)
        assert lib.dwgsim_hip_set_truth_md(ctx.h, 0) == ERR_STATE      # a slot is pending
        ctx.wait(1)
        ctx.set_truth_sam(True)
        b = ctx.simulate(h, 0, 50, 0, 0)
        tagged = ctx.fetch(0, api.STREAM_SAM, b.sam_bytes)
        ctx.set_truth_md(False)
        b = ctx.simulate(h, 0, 50, 0, 0)
        plain = ctx.fetch(0, api.STREAM_SAM, b.sam_bytes)
        assert tagged.count(b"\tNM:i:") == 100 and b"NM:i:" not in plain and tagged.count(b"\n") == plain.count(b"\n") == 100
    assert lib.dwgsim_hip_set_truth_md(None, 1) == T.ERR_ARG and lib.dwgsim_hip_job_set_truth_md(None, 1) == T.ERR_ARG
